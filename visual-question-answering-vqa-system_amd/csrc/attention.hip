// Multi-head attention for gfx950 (self: keys masked with -inf, cross: unmasked): forward and backward in a VALU form (fp32 / bf16, any
// head dim) and a bf16 MFMA form, each plain, with an upstream gradient on the saved softmax (_dp), and indexed (many questions per image).
//   attention                 models/text_encoder.py:237-258 ; models/cross_attention.py:176-198
// q/k/v/ctx are token-major with row strides ld* (elements); head h occupies columns [h*hd, (h+1)*hd).  probs [B][H][Lq][Lk] fp32 holds
// the softmax BEFORE dropout; the backward regenerates the dropout mask from (seed, index).
// ONE text per form: a forward and a backward kernel template per family; the plain backward is the indexed one with a single question
// whose K / V are its own batch's and whose dK / dV sums start at zero.  Each kernel carves its dynamic LDS from the layout struct its
// launcher sizes the launch from (AttnValuLds, AttnFwdLds, AttnBwdLds), so a size is never written twice.
#include <type_traits>
#include "common.h"

// ---------------------------------------------------------------------------------------------
// VALU form, one workgroup of four waves per (batch, head).
// LDS tiles in floats for (Lq, Lk, hd), in this order: Q [Lq][hd+1], (BWD: dctx [Lq][hd+1],) K, V [Lk][hd+1], P [Lq][Lk+1] (BWD: dS
// [Lq][Lk+1]).  The kernels step through the tiles by these sizes, tile pointer from tile pointer (with offsets from the LDS base
// instead the indexed backward needs twice the registers: profiles/attention_ab.txt B); the launchers request floats() and refuse more
// than 160 KiB.  I = int in the kernels, size_t in the launchers.
// ---------------------------------------------------------------------------------------------
template <bool BWD, typename I>
struct AttnValuLds {
  I ldh, ldp, qo, kv, pd;                          // row strides; floats of a Q / dctx tile, of a K / V tile, of a P / dS tile
  __host__ __device__ AttnValuLds(I Lq, I Lk, I hd) : ldh(hd + 1), ldp(Lk + 1), qo(Lq * ldh), kv(Lk * ldh), pd(Lq * ldp) {}
  __host__ __device__ I floats() const { return (BWD ? 2 : 1) * (qo + pd) + 2 * kv; }
};

// IDX (vqa_attention_fwd_idx, _idx_train): the K / V / kmask rows of query batch b are those of image kv_index[b] (n_kv images of
// Lk rows each); an index outside [0, n_kv) loads nothing and writes NaN to that batch's probs and ctx rows.
template <typename T, bool IDX = false>
__global__ __launch_bounds__(256) void attn_fwd_kernel(const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v,
                                                      int ldq, int ldk, int ldv, const float* __restrict__ kmask, float* __restrict__ probs,
                                                      T* __restrict__ ctx, int ldc, int H, int Lq, int Lk, int hd, float scale, float p, uint64_t seed,
                                                      const int* __restrict__ kv_index, int n_kv) {
  seed = drop_resolve(seed);                        // (a flagged seed word names the step-state block: common.h)
  extern __shared__ float sm[];
  const int b = blockIdx.x / H, h = blockIdx.x - b * H, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int kb = b;                                                        // batch of the K / V / kmask rows
  if constexpr (IDX) {
    kb = kv_index[b];
    if (kb < 0 || kb >= n_kv) {                                      // whole block leaves together (before any barrier)
      for (int i = tid; i < Lq * Lk; i += 256) probs[((size_t)(b * H + h) * Lq) * Lk + i] = NAN;
      for (int i = tid; i < Lq * hd; i += 256) { const int r = i / hd, d = i - r * hd; ctx[(size_t)(b * Lq + r) * ldc + h * hd + d] = from_f<T>(NAN); }
      return;
    }
  }
  const AttnValuLds<false, int> lds(Lq, Lk, hd);
  const int ldh = lds.ldh, ldp = lds.ldp;
  float* Qs = sm; float* Ks = Qs + lds.qo; float* Vs = Ks + lds.kv; float* Ps = Vs + lds.kv;
  for (int i = tid; i < Lq * hd; i += 256) { const int r = i / hd, d = i - r * hd; Qs[r * ldh + d] = to_f<T>(q[(size_t)(b * Lq + r) * ldq + h * hd + d]); }
  for (int i = tid; i < Lk * hd; i += 256) {
    const int r = i / hd, d = i - r * hd;
    Ks[r * ldh + d] = to_f<T>(k[(size_t)(kb * Lk + r) * ldk + h * hd + d]);
    Vs[r * ldh + d] = to_f<T>(v[(size_t)(kb * Lk + r) * ldv + h * hd + d]);
  }
  __syncthreads();
  for (int i = tid; i < Lq * Lk; i += 256) {
    const int r = i / Lk, c = i - r * Lk;
    float s = 0.f;
    for (int d = 0; d < hd; ++d) s += Qs[r * ldh + d] * Ks[c * ldh + d];
    s = s / scale;                                                  // divide by sqrt(hd) before masking
    if (kmask && kmask[kb * Lk + c] == 0.f) s = -INFINITY;
    Ps[r * ldp + c] = s;
  }
  __syncthreads();
  float* pg = probs + ((size_t)(b * H + h) * Lq) * Lk;
  for (int r = wave; r < Lq; r += 4) {
    float m = -INFINITY;
    for (int c = lane; c < Lk; c += 64) m = fmaxf(m, Ps[r * ldp + c]);
    m = wave_max(m);
    float sum = 0.f;
    for (int c = lane; c < Lk; c += 64) { const float e = expf(Ps[r * ldp + c] - m); Ps[r * ldp + c] = e; sum += e; }   // all -inf row -> NaN like torch
    sum = wave_sum(sum);
    for (int c = lane; c < Lk; c += 64) {
      float pr = Ps[r * ldp + c] / sum;
      pg[(size_t)r * Lk + c] = pr;
      if (p > 0.f) pr = drop_keep32(drop_key(seed), (uint32_t)(((size_t)(b * H + h) * Lq + r) * Lk + c), p) ? pr / (1.f - p) : 0.f;
      Ps[r * ldp + c] = pr;
    }
  }
  __syncthreads();
  for (int i = tid; i < Lq * hd; i += 256) {
    const int r = i / hd, d = i - r * hd;
    float a = 0.f;
    for (int c = 0; c < Lk; ++c) a += Ps[r * ldp + c] * Vs[c * ldh + d];
    ctx[(size_t)(b * Lq + r) * ldc + h * hd + d] = from_f<T>(a);
  }
}

// The three VALU forward entries: kv_index == nullptr is the plain form.
static int attention_fwd_valu(int dtype, const void* q, const void* k, const void* v, int ldq, int ldk, int ldv, const float* kmask, float* probs,
                              void* ctx, int ldc, int B, int H, int Lq, int Lk, int hd, float p, unsigned long long seed, const int* kv_index,
                              int n_kv, hipStream_t st) {
  const size_t shm = AttnValuLds<false, size_t>(Lq, Lk, hd).floats() * 4;
  if (shm > 160 * 1024) return VQA_EARG;
  const float scale = sqrtf((float)hd);
  auto go = [&](auto kf, auto kb) {
    (void)vqa_ensure_lds(dtype ? reinterpret_cast<const void*>(kb) : reinterpret_cast<const void*>(kf), shm);
    DT(hipLaunchKernelGGL(kf, dim3(B * H), dim3(256), shm, st, (const float*)q, (const float*)k, (const float*)v, ldq, ldk, ldv, kmask, probs, (float*)ctx, ldc, H, Lq, Lk, hd, scale, p, seed, kv_index, n_kv),
       hipLaunchKernelGGL(kb, dim3(B * H), dim3(256), shm, st, (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, ldq, ldk, ldv, kmask, probs, (bf16_t*)ctx, ldc, H, Lq, Lk, hd, scale, p, seed, kv_index, n_kv));
  };
  if (kv_index) go(&attn_fwd_kernel<float, true>, &attn_fwd_kernel<bf16_t, true>);
  else go(&attn_fwd_kernel<float, false>, &attn_fwd_kernel<bf16_t, false>);
  VQA_LAUNCH_CHECK(); return VQA_OK;
}

// One question's contribution to dK[c][d] (a) and dV[c][d] (e), added in query order.
__device__ __forceinline__ void attn_dkdv_add(const float* Ds, const float* Ps, const float* Qs, const float* Os, int Lq, int ldp, int ldh,
                                              int c, int d, float& a, float& e) {
  for (int r = 0; r < Lq; ++r) { a += Ds[r * ldp + c] * Qs[r * ldh + d]; e += Ps[r * ldp + c] * Os[r * ldh + d]; }
}

// Backward.  NACC == 0 (vqa_attention_bwd, _bwd_dp): blockIdx = (batch, head), one question: the batch itself.
// NACC > 0 (vqa_attention_bwd_idx): blockIdx = (image u, head); the block sweeps the image's questions in CSR order (offsets / order
// from vqa_index_csr, N questions) and keeps the image's dK / dV in NACC fp32 accumulators per thread and tensor
// (Lk * hd <= 256 * NACC) that are rounded and stored once; dQ goes to each question's rows.
// DPR: dprobs [B][H][Lq][Lk] (fp32, like probs) is an upstream gradient on the saved softmax, added to dP before the row sums
// (vqa_attention_bwd_dp); read per (q, k) pair along the rows exactly like probs (lane = key: coalesced).
template <typename T, bool DPR, int NACC>
__global__ __launch_bounds__(256) void attn_bwd_kernel(const T* __restrict__ dctx, int ldc, const T* __restrict__ q, const T* __restrict__ k,
                                                      const T* __restrict__ v, int ldq, int ldk, int ldv, const float* __restrict__ probs,
                                                      T* __restrict__ dq, T* __restrict__ dk, T* __restrict__ dv, int lddq, int lddk, int lddv,
                                                      int H, int Lq, int Lk, int hd, float scale, float p, uint64_t seed,
                                                      const int* __restrict__ offsets, const int* __restrict__ order, int N,
                                                      const float* __restrict__ dprobs) {   // (dprobs last: the indexed forms keep seed | offsets adjacent, profiles/attention_ab.txt B.5)
  constexpr bool IDX = NACC > 0;
  static_assert(!(DPR && IDX), "no indexed form with dprobs");
  seed = drop_resolve(seed);                        // (a flagged seed word names the step-state block: common.h)
  extern __shared__ float sm[];
  const int u = blockIdx.x / H, h = blockIdx.x - u * H, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;     // u: batch of the K / V rows
  const AttnValuLds<true, int> lds(Lq, Lk, hd);
  const int ldh = lds.ldh, ldp = lds.ldp;
  float* Qs = sm; float* Os = Qs + lds.qo; float* Ks = Os + lds.qo; float* Vs = Ks + lds.kv;
  float* Ps = Vs + lds.kv; float* Ds = Ps + lds.pd;                 // Ps: dropped probs, Ds: dS
  const int nkd = Lk * hd;
  int beg = 0, end = 1;                       // plain: one question, the block's / wave's own batch
  if constexpr (IDX) {
    beg = offsets[u]; end = offsets[u + 1];
    if (beg < 0 || end < beg || end > N) {        // CSR status error (an index out of range): NaN, never a wrong sum
      for (int i = tid; i < nkd; i += 256) {
        const int c = i / hd, d = i - c * hd;
        dk[(size_t)(u * Lk + c) * lddk + h * hd + d] = from_f<T>(NAN);
        dv[(size_t)(u * Lk + c) * lddv + h * hd + d] = from_f<T>(NAN);
      }
      return;
    }
  }
  if constexpr (IDX) {                          // K / V of image u: once for all its questions
    for (int i = tid; i < nkd; i += 256) {
      const int r = i / hd, d = i - r * hd;
      Ks[r * ldh + d] = to_f<T>(k[(size_t)(u * Lk + r) * ldk + h * hd + d]);
      Vs[r * ldh + d] = to_f<T>(v[(size_t)(u * Lk + r) * ldv + h * hd + d]);
    }
  }
  float ak[IDX ? NACC : 1], av[IDX ? NACC : 1];
#pragma unroll
  for (int jj = 0; jj < NACC; ++jj) { ak[jj] = 0.f; av[jj] = 0.f; }
  // The questions.  Plain: `IDX && ...` is compile-time false, the body is straight-line code.  NOT a for loop: around the plain body
  // a for loop, even one with the constant bounds 0 and 1, costs the backward kernels registers and scratch (profiles/attention_ab.txt B.1).
  int jq = beg;
  if (!IDX || jq < end) do {
    int b = u;
    if constexpr (IDX) {
      b = order[jq];
      if (b < 0 || b >= N) continue;              // block-uniform
      __syncthreads();                            // the previous question's readers of Qs / Os / Ps / Ds are done
    }
    for (int i = tid; i < Lq * hd; i += 256) {
      const int r = i / hd, d = i - r * hd;
      Qs[r * ldh + d] = to_f<T>(q[(size_t)(b * Lq + r) * ldq + h * hd + d]);
      Os[r * ldh + d] = to_f<T>(dctx[(size_t)(b * Lq + r) * ldc + h * hd + d]);
    }
    if constexpr (!IDX) {                       // plain: K / V behind Q / dctx, the order these loads always had (profiles/attention_ab.txt B.6)
      for (int i = tid; i < nkd; i += 256) {
        const int r = i / hd, d = i - r * hd;
        Ks[r * ldh + d] = to_f<T>(k[(size_t)(u * Lk + r) * ldk + h * hd + d]);
        Vs[r * ldh + d] = to_f<T>(v[(size_t)(u * Lk + r) * ldv + h * hd + d]);
      }
    }
    __syncthreads();
    const float* pg = probs + ((size_t)(b * H + h) * Lq) * Lk;
    for (int r = wave; r < Lq; r += 4) {
      float t = 0.f;
      for (int c = lane; c < Lk; c += 64) {
        const float pr = pg[(size_t)r * Lk + c];
        float ks = 1.f;
        if (p > 0.f) ks = drop_keep32(drop_key(seed), (uint32_t)(((size_t)(b * H + h) * Lq + r) * Lk + c), p) ? 1.f / (1.f - p) : 0.f;
        float dpd = 0.f;
        for (int d = 0; d < hd; ++d) dpd += Os[r * ldh + d] * Vs[c * ldh + d];
        float dp = dpd * ks;
        if constexpr (DPR) dp += dprobs[((size_t)(b * H + h) * Lq + r) * Lk + c];
        Ps[r * ldp + c] = pr * ks;
        Ds[r * ldp + c] = dp;
        t += dp * pr;
      }
      t = wave_sum(t);
      for (int c = lane; c < Lk; c += 64) Ds[r * ldp + c] = pg[(size_t)r * Lk + c] * (Ds[r * ldp + c] - t) / scale;
    }
    __syncthreads();
    for (int i = tid; i < Lq * hd; i += 256) {
      const int r = i / hd, d = i - r * hd;
      float a = 0.f;
      for (int c = 0; c < Lk; ++c) a += Ds[r * ldp + c] * Ks[c * ldh + d];
      dq[(size_t)(b * Lq + r) * lddq + h * hd + d] = from_f<T>(a);
    }
    if constexpr (IDX) {
#pragma unroll
      for (int jj = 0; jj < NACC; ++jj) {
        const int i = tid + jj * 256;
        if (i < nkd) {
          const int c = i / hd, d = i - c * hd;
          float a = ak[jj], e = av[jj];
          attn_dkdv_add(Ds, Ps, Qs, Os, Lq, ldp, ldh, c, d, a, e);
          ak[jj] = a; av[jj] = e;
        }
      }
    } else {
      for (int i = tid; i < nkd; i += 256) {      // one question: sum, round and store in one go, any Lk * hd
        const int c = i / hd, d = i - c * hd;
        float a = 0.f, e = 0.f;
        attn_dkdv_add(Ds, Ps, Qs, Os, Lq, ldp, ldh, c, d, a, e);
        dk[(size_t)(u * Lk + c) * lddk + h * hd + d] = from_f<T>(a);
        dv[(size_t)(u * Lk + c) * lddv + h * hd + d] = from_f<T>(e);
      }
    }
  } while (IDX && ++jq < end);
#pragma unroll
  for (int jj = 0; jj < NACC; ++jj) {
    const int i = tid + jj * 256;
    if (i < nkd) {
      const int c = i / hd, d = i - c * hd;
      dk[(size_t)(u * Lk + c) * lddk + h * hd + d] = from_f<T>(ak[jj]);
      dv[(size_t)(u * Lk + c) * lddv + h * hd + d] = from_f<T>(av[jj]);
    }
  }
}

// nblk = B * H (plain, _dp) or n_kv * H (indexed)
template <bool DPR, int NACC>
static int attention_bwd_valu(int dtype, const void* dctx, int ldc, const void* q, const void* k, const void* v, int ldq, int ldk, int ldv,
                              const float* probs, const float* dprobs, const int* offsets, const int* order, int N, void* dq, void* dk, void* dv,
                              int lddq, int lddk, int lddv, int nblk, int H, int Lq, int Lk, int hd, float p, unsigned long long seed,
                              hipStream_t st) {
  const size_t shm = AttnValuLds<true, size_t>(Lq, Lk, hd).floats() * 4;
  const float scale = sqrtf((float)hd);
  (void)vqa_ensure_lds(dtype ? reinterpret_cast<const void*>(&attn_bwd_kernel<bf16_t, DPR, NACC>) : reinterpret_cast<const void*>(&attn_bwd_kernel<float, DPR, NACC>), shm);
  DT(hipLaunchKernelGGL((attn_bwd_kernel<float, DPR, NACC>), dim3(nblk), dim3(256), shm, st, (const float*)dctx, ldc, (const float*)q, (const float*)k, (const float*)v, ldq, ldk, ldv, probs, (float*)dq, (float*)dk, (float*)dv, lddq, lddk, lddv, H, Lq, Lk, hd, scale, p, seed, offsets, order, N, dprobs),
     hipLaunchKernelGGL((attn_bwd_kernel<bf16_t, DPR, NACC>), dim3(nblk), dim3(256), shm, st, (const bf16_t*)dctx, ldc, (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, ldq, ldk, ldv, probs, (bf16_t*)dq, (bf16_t*)dk, (bf16_t*)dv, lddq, lddk, lddv, H, Lq, Lk, hd, scale, p, seed, offsets, order, N, dprobs));
  VQA_LAUNCH_CHECK(); return VQA_OK;
}
static bool attn_bwd_valu_fits(int Lq, int Lk, int hd) { return AttnValuLds<true, size_t>(Lq, Lk, hd).floats() * 4 <= 160 * 1024; }

// ---------------------------------------------------------------------------------------------
// bf16 MFMA form: one wave per (batch, head), Lq <= 32 queries, Lk <= 32 * NKT keys, head dim HD in {32, 64}.
// NKT = key tiles of 32 (2: Lk <= 64, the 49 image tokens / 20 text tokens; 5: Lk <= 160, the 144 image tokens of the 384x384
// stress shape), WPB = waves (= (batch, head) problems) per workgroup, all LDS wave-private (no block barrier anywhere).
// ---------------------------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(16))) float f32x16;

// (hd, Lk) -> f(<HD>, <NKT>) for hd in {32, 64}, Lk <= 160
template <int V> using attn_ic = std::integral_constant<int, V>;
template <typename F>
static void attn_mfma_tile(int hd, int Lk, F f) {
  if (Lk <= 64) { if (hd == 32) f(attn_ic<32>{}, attn_ic<2>{}); else f(attn_ic<64>{}, attn_ic<2>{}); }
  else { if (hd == 32) f(attn_ic<32>{}, attn_ic<5>{}); else f(attn_ic<64>{}, attn_ic<5>{}); }
}
// row (orientation: key or query) of accumulator register e of a 32x32 MFMA tile in the lane's half hh; its column is lane & 31
__device__ __forceinline__ int attn_acc_row(int e, int hh) { return (e & 3) + 8 * (e >> 2) + 4 * hh; }
// The n rows of batch b, head h of src -> LDS tile [ROWS][HD] as 16-byte vectors, padding rows (>= n) zero.  A macro, not a function
// (and the backward's two-tensor form of it stays written out): with either as an inlined function attn_bwd_mfma_kernel<32, 5, 2, DPR =
// true>, which sits at the register ceiling, spills one more register (profiles/attention_ab.txt B).
#define ATTN_STAGE_ROWS(HD, lane, tile, ROWS, src, ld, b, n, h)                                                                \
  for (int i = (lane); i < (ROWS) * (HD / 8); i += 64) {                                                                      \
    const int row = i / (HD / 8), cv = i - row * (HD / 8);                                                                    \
    u32x4 val = {0u, 0u, 0u, 0u};                                                                                             \
    if (row < (n)) val = *reinterpret_cast<const u32x4*>((src) + (size_t)((b) * (n) + row) * (ld) + (h) * HD + cv * 8);       \
    *reinterpret_cast<u32x4*>(&(tile)[row * HD + cv * 8]) = val;                                                              \
  }
// B operand of the MFMA that follows one whose bf16-rounded accumulators are the A operand: tile rows row0.., read transposed in the
// matching (permuted) k order
template <int HD>
__device__ __forceinline__ bf16x8 attn_ldsB(const bf16_t* tile, int row0, int c, int hh, int g2, int qd, int pp) {
  typedef __attribute__((ext_vector_type(8))) short i16x8;
  const bf16_t* vb = tile + (row0 + 4 * hh + qd) * HD + c * 32 + 16 * g2 + 4 * pp;
  i16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((i16x4 __attribute__((address_space(3)))*)(vb));
  i16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((i16x4 __attribute__((address_space(3)))*)(vb + 8 * HD));
  i16x8 tt = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, tt);
}

// Forward:
//   S^T (keys x queries) = K . Q^T         v_mfma_f32_32x32x16_bf16, operands loaded straight from global as 16-byte fragments
//   row softmax over keys: the query sits on the lane, its keys in the 32 accumulator registers of the two key tiles
//     (+ one exchange with lane^32); probabilities go to the caller through an LDS staging tile (coalesced rows)
//   ctx = P . V = (P^T)^T . V: the bf16-rounded accumulator registers ARE the A operand of the next MFMA (no lane movement);
//     V is staged in LDS and read transposed with ds_read_b64_tr_b16 in the matching (permuted) k order.
// Same masking semantics as the reference: keys with kmask == 0 get -inf before the softmax (an all-masked row is NaN).
// LDS of a workgroup: WPB V tiles [KR][HD] bf16 (row stride 64 / 128 bytes, 8-byte aligned for the transposed reads), then WPB
// probability staging tiles [32][KR + 1] fp32.
template <int HD, int NKT, int WPB>
struct AttnFwdLds {
  static constexpr int KR = NKT * 32, LDP = KR + 1;
  static constexpr int V_WAVE = KR * HD * 2, P0 = WPB * V_WAVE, P_WAVE = 32 * LDP * 4, BYTES = P0 + WPB * P_WAVE;
};
// IDX (vqa_attention_fwd_mfma_idx, _idx_train): K / V / kmask rows of image kv_index[b] (n_kv images); out of range -> NaN rows.
template <int HD, int NKT, int WPB, bool IDX = false>
__global__ __launch_bounds__(WPB * 64, 1) void attn_fwd_mfma_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k, const bf16_t* __restrict__ v,
                                                            int ldq, int ldk, int ldv, const float* __restrict__ kmask, float* __restrict__ probs,
                                                            bf16_t* __restrict__ ctx, int ldc, int BH, int H, int Lq, int Lk, float p, uint64_t seed,
                                                            const int* __restrict__ kv_index, int n_kv) {
  seed = drop_resolve(seed);                        // (a flagged seed word names the step-state block: common.h)
  using Lds = AttnFwdLds<HD, NKT, WPB>;
  constexpr int KR = Lds::KR, LDP = Lds::LDP;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int bh = blockIdx.x * WPB + wave;
  bf16_t* Vs = reinterpret_cast<bf16_t*>(smem + wave * Lds::V_WAVE);
  float* Ps = reinterpret_cast<float*>(smem + Lds::P0 + wave * Lds::P_WAVE);
  if (bh >= BH) return;                         // whole wave exits together; no block-level barrier is used below
  const int b = bh / H, h = bh - b * H;
  const int r = lane & 31, hh = lane >> 5;
  const float inv_scale = 1.0f / sqrtf((float)HD);
  int kb = b;                                   // batch of the K / V / kmask rows
  if constexpr (IDX) {
    kb = __builtin_amdgcn_readfirstlane(kv_index[b]);
    if (kb < 0 || kb >= n_kv) {                 // the whole wave leaves together
      for (int i = lane; i < Lq * Lk; i += 64) probs[(size_t)bh * Lq * Lk + i] = NAN;
      for (int i = lane; i < Lq * HD; i += 64) ctx[(size_t)(b * Lq + i / HD) * ldc + h * HD + i % HD] = f2bf(NAN);
      return;
    }
  }

  ATTN_STAGE_ROWS(HD, lane, Vs, KR, v, ldv, kb, Lk, h)
  // ---- S^T = K Q^T
  f32x16 st[NKT];
#pragma unroll
  for (int t = 0; t < NKT; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) st[t][e] = 0.f;
#pragma unroll
  for (int ks = 0; ks < HD / 16; ++ks) {
    bf16x8 qf = {};
    if (r < Lq) qf = *reinterpret_cast<const bf16x8*>(q + (size_t)(b * Lq + r) * ldq + h * HD + ks * 16 + 8 * hh);
#pragma unroll
    for (int t = 0; t < NKT; ++t) {
      bf16x8 kf = {};
      if (32 * t + r < Lk) kf = *reinterpret_cast<const bf16x8*>(k + (size_t)(kb * Lk + 32 * t + r) * ldk + h * HD + ks * 16 + 8 * hh);
      st[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf, st[t], 0, 0, 0);
    }
  }
  // ---- scale, mask, softmax over keys (query = lane&31; keys: 32*t + attn_acc_row)
  float m = -INFINITY;
#pragma unroll
  for (int t = 0; t < NKT; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int key = 32 * t + attn_acc_row(e, hh);
      float s = st[t][e] * inv_scale;
      if (key >= Lk || (kmask && kmask[kb * Lk + key] == 0.f)) s = -INFINITY;
      st[t][e] = s;
      m = fmaxf(m, s);
    }
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  float sum = 0.f;
#pragma unroll
  for (int t = 0; t < NKT; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) { const float ex = expf(st[t][e] - m); st[t][e] = ex; sum += ex; }   // all -inf row -> NaN like torch
  sum += __shfl_xor(sum, 32, 64);
  const float rs = 1.0f / sum;
  const size_t prow = ((size_t)bh * Lq + r) * Lk;
#pragma unroll
  for (int t = 0; t < NKT; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int key = 32 * t + attn_acc_row(e, hh);
      float pr = st[t][e] * rs;
      if (sum != sum || m != m) pr = st[t][e] / sum;                       // keep NaN propagation exact (0 * inf etc.)
      Ps[r * LDP + key] = pr;
      if (p > 0.f && r < Lq && key < Lk) pr = drop_keep32(drop_key(seed), (uint32_t)(prow + key), p) ? pr / (1.f - p) : 0.f;
      st[t][e] = pr;
    }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                     // wave-private LDS: V tile + probabilities are visible
  for (int i = lane; i < Lq * Lk; i += 64) { const int qi = i / Lk, kj = i - qi * Lk; probs[(size_t)bh * Lq * Lk + i] = Ps[qi * LDP + kj]; }
  // ---- ctx = P V : A operand = bf16(accumulator registers 8s..8s+7), B operand = V rows in the matching permuted key order
  f32x16 o[HD / 32];
#pragma unroll
  for (int c = 0; c < HD / 32; ++c)
#pragma unroll
    for (int e = 0; e < 16; ++e) o[c][e] = 0.f;
  const int g2 = (lane >> 4) & 1, li = lane & 15, qd = li >> 2, pp = li & 3;
#pragma unroll
  for (int t = 0; t < NKT; ++t)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bf16x8 af;
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) af[jj] = (__bf16)st[t][8 * s + jj];
#pragma unroll
      for (int c = 0; c < HD / 32; ++c)
        o[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, attn_ldsB<HD>(Vs, 32 * t + 16 * s, c, hh, g2, qd, pp), o[c], 0, 0, 0);
    }
#pragma unroll
  for (int c = 0; c < HD / 32; ++c)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int qi = attn_acc_row(e, hh);
      if (qi < Lq) ctx[(size_t)(b * Lq + qi) * ldc + h * HD + c * 32 + r] = f2bf(o[c][e]);
    }
}

// The three MFMA forward entries: kv_index == nullptr is the plain form.
static int attention_fwd_mfma(const void* q, const void* k, const void* v, int ldq, int ldk, int ldv, const float* kmask, float* probs, void* ctx,
                              int ldc, int B, int H, int Lq, int Lk, int hd, float p, unsigned long long seed, const int* kv_index, int n_kv,
                              hipStream_t st) {
  if (!q || !k || !v || !probs || !ctx || Lq > 32 || Lk > 160 || (hd != 32 && hd != 64) || (ldq % 8) || (ldk % 8) || (ldv % 8)) return VQA_EARG;
  const int BH = B * H;
  attn_mfma_tile(hd, Lk, [&](auto hd_, auto nkt_) {
    constexpr int HD = decltype(hd_)::value, NKT = decltype(nkt_)::value, WPB = NKT == 2 ? 4 : 2;    // the NKT = 5 tiles fit two per CU
    constexpr size_t shm = AttnFwdLds<HD, NKT, WPB>::BYTES;
    auto go = [&](auto kern) {
      (void)vqa_ensure_lds(reinterpret_cast<const void*>(kern), shm);
      hipLaunchKernelGGL(kern, dim3((BH + WPB - 1) / WPB), dim3(WPB * 64), shm, st, (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, ldq, ldk, ldv,
                         kmask, probs, (bf16_t*)ctx, ldc, BH, H, Lq, Lk, p, seed, kv_index, n_kv);
    };
    if (kv_index) go(&attn_fwd_mfma_kernel<HD, NKT, WPB, true>); else go(&attn_fwd_mfma_kernel<HD, NKT, WPB, false>);
  });
  VQA_LAUNCH_CHECK(); return VQA_OK;
}

// Backward.  dP is formed TWICE from the same global 16-byte fragments (MFMAs are free at this size):
//   orientation 1  dP^T = V . dctx^T   (lane = query, registers = keys)   -> row sums t[q], dS -> dQ = dS . K
//   orientation 2  dP   = dctx . V^T   (lane = key,   registers = queries) -> dS, dropped P  -> dK = dS^T . Q, dV = Pd^T . dctx
// In both, the bf16-rounded accumulator registers are the A operand of the following MFMA (as in the forward kernel) and the
// B operand (K, Q or dctx rows) is read transposed from a wave-private LDS tile in the matching permuted order.
// DPR (vqa_attention_bwd_mfma_dp): dprobs [B][H][Lq][Lk] fp32, an upstream gradient on the saved softmax, is staged in a wave-private LDS
// tile by the same coalesced row copy as probs and added to dP in both orientations: dP = ks * (dctx V^T) + dprobs.
// IDX (vqa_attention_bwd_mfma_idx): the wave owns (image u, head h) and sweeps the image's questions in CSR order (offsets / order from
// vqa_index_csr, N questions): dQ per question; the fp32 dK / dV accumulators live in a wave-private LDS area in the MFMA accumulator
// layout, lane-private ([tile][c][e][lane]: no bank conflicts, no cross-lane traffic); each question's orientation-2 MFMAs start from
// them instead of from zero, and they are rounded and stored once at the end.  An image without questions gets zeros.
// Plain: one question, the wave's own batch; orientation 2 starts from zero in registers and stores straight away.
// LDS of one wave, in bytes: K [KR][HD], Q [32][HD], dctx [32][HD] bf16; P [32][KR + 1], t [32] fp32; then dprobs [32][KR + 1] (DPR)
// or the dK and dV accumulators [NACC][64] (IDX).
template <int HD, int NKT, bool DPR, bool IDX>
struct AttnBwdLds {
  static_assert(!(DPR && IDX), "no indexed form with dprobs");
  static constexpr int KR = NKT * 32, LDP = KR + 1;
  static constexpr int NACC = NKT * (HD / 32) * 16;     // accumulator registers per lane and tensor
  static constexpr int K = 0, Q = K + KR * HD * 2, O = Q + 32 * HD * 2, P = O + 32 * HD * 2, T = P + 32 * LDP * 4, X = T + 32 * 4;
  static constexpr int DP = X, AK = X, AV = AK + NACC * 64 * 4;
  static constexpr int WAVE_BYTES = X + (DPR ? 32 * LDP * 4 : 0) + (IDX ? 2 * NACC * 64 * 4 : 0);
};
template <int HD, int NKT, int WPB, bool DPR, bool IDX>
__global__ __launch_bounds__(WPB * 64, 1) void attn_bwd_mfma_kernel(const bf16_t* __restrict__ dctx, int ldc, const bf16_t* __restrict__ q,
                                                            const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, int ldq, int ldk, int ldv,
                                                            const float* __restrict__ probs, bf16_t* __restrict__ dq, bf16_t* __restrict__ dk,
                                                            bf16_t* __restrict__ dv, int lddq, int lddk, int lddv, int UH, int H, int Lq, int Lk,
                                                            float p, uint64_t seed, const float* __restrict__ dprobs,
                                                            const int* __restrict__ offsets, const int* __restrict__ order, int N) {
  seed = drop_resolve(seed);                        // (a flagged seed word names the step-state block: common.h)
  using Lds = AttnBwdLds<HD, NKT, DPR, IDX>;
  constexpr int KR = Lds::KR, LDP = Lds::LDP, NACC = Lds::NACC;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int uh = blockIdx.x * WPB + wave;
  if (uh >= UH) return;                         // whole wave exits together; only wave-private LDS, no block barrier below
  char* base = smem + (size_t)wave * Lds::WAVE_BYTES;
  bf16_t* Ks = reinterpret_cast<bf16_t*>(base + Lds::K);
  bf16_t* Qs = reinterpret_cast<bf16_t*>(base + Lds::Q);
  bf16_t* Os = reinterpret_cast<bf16_t*>(base + Lds::O);   // dctx
  float* Ps = reinterpret_cast<float*>(base + Lds::P);
  float* Ts = reinterpret_cast<float*>(base + Lds::T);
  float* DPs = reinterpret_cast<float*>(base + Lds::DP);   // DPR only
  float* Ak = reinterpret_cast<float*>(base + Lds::AK);    // IDX only
  float* Av = reinterpret_cast<float*>(base + Lds::AV);
  const int u = uh / H, h = uh - u * H;         // u: batch (plain) / image (IDX) of the K / V rows
  const int r = lane & 31, hh = lane >> 5;
  const int g2 = (lane >> 4) & 1, li = lane & 15, qd = li >> 2, pp = li & 3;
  const float inv_scale = 1.0f / sqrtf((float)HD);
  const float keep = p > 0.f ? 1.f / (1.f - p) : 1.f;
  int beg = 0, end = 1;                       // plain: one question, the block's / wave's own batch
  if constexpr (IDX) {
    beg = __builtin_amdgcn_readfirstlane(offsets[u]); end = __builtin_amdgcn_readfirstlane(offsets[u + 1]);
    if (beg < 0 || end < beg || end > N) {        // CSR status error (an index out of range): NaN, never a wrong sum
      for (int i = lane; i < Lk * HD; i += 64) {
        const int c = i / HD, d = i - c * HD;
        dk[(size_t)(u * Lk + c) * lddk + h * HD + d] = f2bf(NAN);
        dv[(size_t)(u * Lk + c) * lddv + h * HD + d] = f2bf(NAN);
      }
      return;
    }
  }
  ATTN_STAGE_ROWS(HD, lane, Ks, KR, k, ldk, u, Lk, h)
  if constexpr (IDX)
    for (int i = 0; i < NACC; ++i) { Ak[i * 64 + lane] = 0.f; Av[i * 64 + lane] = 0.f; }

  // The questions.  Plain: `IDX && ...` is compile-time false, the body is straight-line code.  NOT a for loop: around the plain body
  // a for loop, even one with the constant bounds 0 and 1, costs the backward kernels registers and scratch (profiles/attention_ab.txt B.1).
  int jq = beg;
  if (!IDX || jq < end) do {
    int b = u;
    if constexpr (IDX) {
      b = __builtin_amdgcn_readfirstlane(order[jq]);
      if (b < 0 || b >= N) continue;              // wave-uniform
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // the previous question's LDS reads are complete
    }
    const int bh = b * H + h;                   // the question's (batch, head): probs, dropout index, dQ
    // ---- Q, dctx -> LDS (16-byte vectors, padding rows zero); probabilities -> LDS
    for (int i = lane; i < 32 * (HD / 8); i += 64) {
      const int row = i / (HD / 8), cv = i - row * (HD / 8);
      u32x4 a = {0u, 0u, 0u, 0u}, o = {0u, 0u, 0u, 0u};
      if (row < Lq) {
        a = *reinterpret_cast<const u32x4*>(q + (size_t)(b * Lq + row) * ldq + h * HD + cv * 8);
        o = *reinterpret_cast<const u32x4*>(dctx + (size_t)(b * Lq + row) * ldc + h * HD + cv * 8);
      }
      *reinterpret_cast<u32x4*>(&Qs[row * HD + cv * 8]) = a;
      *reinterpret_cast<u32x4*>(&Os[row * HD + cv * 8]) = o;
    }
    for (int i = lane; i < Lq * Lk; i += 64) { const int qi = i / Lk, kj = i - qi * Lk; Ps[qi * LDP + kj] = probs[(size_t)bh * Lq * Lk + i]; }
    if constexpr (DPR)
      for (int i = lane; i < Lq * Lk; i += 64) { const int qi = i / Lk, kj = i - qi * Lk; DPs[qi * LDP + kj] = dprobs[(size_t)bh * Lq * Lk + i]; }

    // ---- both orientations of dP = dctx V^T from the same global fragments
    f32x16 d1[NKT], d2[NKT];
#pragma unroll
    for (int t = 0; t < NKT; ++t)
#pragma unroll
      for (int e = 0; e < 16; ++e) { d1[t][e] = 0.f; d2[t][e] = 0.f; }
#pragma unroll
    for (int ks = 0; ks < HD / 16; ++ks) {
      bf16x8 of = {};
      if (r < Lq) of = *reinterpret_cast<const bf16x8*>(dctx + (size_t)(b * Lq + r) * ldc + h * HD + ks * 16 + 8 * hh);
#pragma unroll
      for (int t = 0; t < NKT; ++t) {
        bf16x8 vf = {};
        if (32 * t + r < Lk) vf = *reinterpret_cast<const bf16x8*>(v + (size_t)(u * Lk + 32 * t + r) * ldv + h * HD + ks * 16 + 8 * hh);
        d1[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, of, d1[t], 0, 0, 0);      // rows = keys, cols = queries
        d2[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(of, vf, d2[t], 0, 0, 0);      // rows = queries, cols = keys
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                     // LDS tiles written above are visible to the whole wave

    // ---- orientation 1: query = r, keys = 32t + attn_acc_row: row sums, dS, dQ = dS K
    const size_t prow = ((size_t)bh * Lq + r) * Lk;
    float tq = 0.f;
#pragma unroll
    for (int t = 0; t < NKT; ++t)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int key = 32 * t + attn_acc_row(e, hh);
        const bool ok = r < Lq && key < Lk;
        const float pr = ok ? Ps[r * LDP + key] : 0.f;
        float ks = 1.f;
        if (p > 0.f && ok) ks = drop_keep32(drop_key(seed), (uint32_t)(prow + key), p) ? keep : 0.f;
        float dp = ok ? d1[t][e] * ks : 0.f;
        if constexpr (DPR) dp += ok ? DPs[r * LDP + key] : 0.f;
        tq += dp * pr;
        d1[t][e] = dp;
      }
    tq += __shfl_xor(tq, 32, 64);
    if (hh == 0) Ts[r] = tq;
#pragma unroll
    for (int t = 0; t < NKT; ++t)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int key = 32 * t + attn_acc_row(e, hh);
        const float pr = (r < Lq && key < Lk) ? Ps[r * LDP + key] : 0.f;
        d1[t][e] = pr * (d1[t][e] - tq) * inv_scale;                     // dS[query r][key]
      }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    f32x16 oq[HD / 32];
#pragma unroll
    for (int c = 0; c < HD / 32; ++c)
#pragma unroll
      for (int e = 0; e < 16; ++e) oq[c][e] = 0.f;
#pragma unroll
    for (int t = 0; t < NKT; ++t)
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        bf16x8 af;
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) af[jj] = (__bf16)d1[t][8 * s2 + jj];
#pragma unroll
        for (int c = 0; c < HD / 32; ++c)
          oq[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, attn_ldsB<HD>(Ks, 32 * t + 16 * s2, c, hh, g2, qd, pp), oq[c], 0, 0, 0);
      }
#pragma unroll
    for (int c = 0; c < HD / 32; ++c)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int qi = attn_acc_row(e, hh);
        if (qi < Lq) dq[(size_t)(b * Lq + qi) * lddq + h * HD + c * 32 + r] = f2bf(oq[c][e]);
      }

    // ---- orientation 2: key = 32t + r, queries = attn_acc_row ; dK (+)= dS^T Q, dV (+)= Pd^T dctx
#pragma unroll
    for (int t = 0; t < NKT; ++t) {
      const int key = 32 * t + r;
      f32x16 ds2, pd2;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int qi = attn_acc_row(e, hh);
        const bool ok = qi < Lq && key < Lk;
        const float pr = ok ? Ps[qi * LDP + key] : 0.f;
        float ks = 1.f;
        if (p > 0.f && ok) ks = drop_keep32(drop_key(seed), (uint32_t)(((size_t)bh * Lq + qi) * Lk + key), p) ? keep : 0.f;
        float dp = ok ? d2[t][e] * ks : 0.f;
        if constexpr (DPR) dp += ok ? DPs[qi * LDP + key] : 0.f;
        const float tt = ok ? Ts[qi] : 0.f;
        ds2[e] = pr * (dp - tt) * inv_scale;
        pd2[e] = pr * ks;
      }
      f32x16 okk[HD / 32], ovv[HD / 32];
#pragma unroll
      for (int c = 0; c < HD / 32; ++c)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          if constexpr (IDX) {
            const int a = ((t * (HD / 32) + c) * 16 + e) * 64 + lane;
            okk[c][e] = Ak[a]; ovv[c][e] = Av[a];
          } else {
            okk[c][e] = 0.f; ovv[c][e] = 0.f;
          }
        }
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        bf16x8 as, ap;
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) { as[jj] = (__bf16)ds2[8 * s2 + jj]; ap[jj] = (__bf16)pd2[8 * s2 + jj]; }
#pragma unroll
        for (int c = 0; c < HD / 32; ++c) {
          okk[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as, attn_ldsB<HD>(Qs, 16 * s2, c, hh, g2, qd, pp), okk[c], 0, 0, 0);
          ovv[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ap, attn_ldsB<HD>(Os, 16 * s2, c, hh, g2, qd, pp), ovv[c], 0, 0, 0);
        }
      }
#pragma unroll
      for (int c = 0; c < HD / 32; ++c)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          if constexpr (IDX) {
            const int a = ((t * (HD / 32) + c) * 16 + e) * 64 + lane;
            Ak[a] = okk[c][e]; Av[a] = ovv[c][e];
          } else {
            const int kj = 32 * t + attn_acc_row(e, hh);
            if (kj < Lk) {
              dk[(size_t)(u * Lk + kj) * lddk + h * HD + c * 32 + r] = f2bf(okk[c][e]);
              dv[(size_t)(u * Lk + kj) * lddv + h * HD + c * 32 + r] = f2bf(ovv[c][e]);
            }
          }
        }
    }
  } while (IDX && ++jq < end);
  if constexpr (IDX) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    for (int t = 0; t < NKT; ++t)
#pragma unroll
      for (int c = 0; c < HD / 32; ++c)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int kj = 32 * t + attn_acc_row(e, hh);
          const int a = ((t * (HD / 32) + c) * 16 + e) * 64 + lane;
          if (kj < Lk) {
            dk[(size_t)(u * Lk + kj) * lddk + h * HD + c * 32 + r] = f2bf(Ak[a]);
            dv[(size_t)(u * Lk + kj) * lddv + h * HD + c * 32 + r] = f2bf(Av[a]);
          }
        }
  }
}

// UH = B * H (plain, _dp) or n_kv * H (IDX); the callers have checked the arguments
template <bool DPR, bool IDX>
static int attention_bwd_mfma(const void* dctx, int ldc, const void* q, const void* k, const void* v, int ldq, int ldk, int ldv,
                              const float* probs, const float* dprobs, const int* offsets, const int* order, int N, void* dq, void* dk, void* dv,
                              int lddq, int lddk, int lddv, int UH, int H, int Lq, int Lk, int hd, float p, unsigned long long seed, hipStream_t st) {
  attn_mfma_tile(hd, Lk, [&](auto hd_, auto nkt_) {
    constexpr int HD = decltype(hd_)::value, NKT = decltype(nkt_)::value;
    constexpr int WPB = (NKT == 2 ? 4 : 2) / (IDX ? 2 : 1);             // the accumulator area of the indexed form halves the waves that fit
    constexpr size_t shm = (size_t)WPB * AttnBwdLds<HD, NKT, DPR, IDX>::WAVE_BYTES;
    auto kern = &attn_bwd_mfma_kernel<HD, NKT, WPB, DPR, IDX>;
    (void)vqa_ensure_lds(reinterpret_cast<const void*>(kern), shm);
    hipLaunchKernelGGL(kern, dim3((UH + WPB - 1) / WPB), dim3(WPB * 64), shm, st, (const bf16_t*)dctx, ldc, (const bf16_t*)q, (const bf16_t*)k,
                       (const bf16_t*)v, ldq, ldk, ldv, probs, (bf16_t*)dq, (bf16_t*)dk, (bf16_t*)dv, lddq, lddk, lddv, UH, H, Lq, Lk, p, seed,
                       dprobs, offsets, order, N);
  });
  VQA_LAUNCH_CHECK(); return VQA_OK;
}
template <bool DPR>
static int attention_bwd_mfma_plain(const void* dctx, int ldc, const void* q, const void* k, const void* v, int ldq, int ldk, int ldv,
                                    const float* probs, const float* dprobs, void* dq, void* dk, void* dv, int lddq, int lddk, int lddv,
                                    int B, int H, int Lq, int Lk, int hd, float p, unsigned long long seed, hipStream_t st) {
  if (!dctx || !q || !k || !v || !probs || !dq || !dk || !dv || (DPR && !dprobs) || Lq > 32 || Lk > 160 || (hd != 32 && hd != 64) ||
      (ldq % 8) || (ldk % 8) || (ldv % 8) || (ldc % 8)) return VQA_EARG;
  return attention_bwd_mfma<DPR, false>(dctx, ldc, q, k, v, ldq, ldk, ldv, probs, dprobs, nullptr, nullptr, 0, dq, dk, dv, lddq, lddk, lddv,
                                        B * H, H, Lq, Lk, hd, p, seed, st);
}

// ---------------------------------------------------------------------------------------------
// Many questions per image in TRAINING (VQAModel.forward_grouped, HipTrainer.step(image_index=)).
//   vqa_index_csr              questions of each image in ascending question order (CSR), one workgroup, no host sync
//   vqa_attention_fwd(_mfma)_idx_train   the indexed forwards with dropout: the mask of (question b, head, i, j) is the one
//                              vqa_attention_fwd(_mfma) draws for batch b (identity index -> bit-equal)
//   vqa_attention_bwd(_mfma)_idx         dQ per question, dK / dV per IMAGE in fp32 accumulators over that image's questions in CSR
//                              order, rounded and stored once.  No float atomics: the sums run in a fixed order (bit-reproducible).
//                              One question per image: the products and their order are those of vqa_attention_bwd(_mfma)
//                              (bit-equal: the same kernel text); an image without questions gets zeros.
// ---------------------------------------------------------------------------------------------

// Counting sort of kv_index [N] into offsets [U+1] / order [N]; cur: U ints of dynamic LDS (counts, then per-image cursors).
// Placement is stable: question i's slot = cursor of its image + #{earlier questions of the same image in its chunk of 1024}.
// An index outside [0, U) writes -1 to every offset and order entry (the status the backward kernels check).
__global__ __launch_bounds__(1024) void index_csr_kernel(const int* __restrict__ kv_index, int N, int U, int* __restrict__ offsets,
                                                         int* __restrict__ order) {
  extern __shared__ int cur[];
  __shared__ int part[1024];
  __shared__ int keys[1024];
  __shared__ int bad;
  const int tid = threadIdx.x;
  if (tid == 0) bad = 0;
  for (int u = tid; u < U; u += 1024) cur[u] = 0;
  __syncthreads();
  for (int i = tid; i < N; i += 1024) {
    const int u = kv_index[i];
    if (u < 0 || u >= U) bad = 1;
    else atomicAdd(&cur[u], 1);                 // integer counts: order-independent
  }
  __syncthreads();
  if (bad) {                                    // block-uniform
    for (int u = tid; u <= U; u += 1024) offsets[u] = -1;
    for (int i = tid; i < N; i += 1024) order[i] = -1;
    return;
  }
  // exclusive scan of the counts: thread t owns images [u0, u1)
  const int per = (U + 1023) / 1024, u0 = min(tid * per, U), u1 = min(u0 + per, U);
  int s = 0;
  for (int u = u0; u < u1; ++u) s += cur[u];
  part[tid] = s;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {          // inclusive scan of the 1024 partial sums
    const int v = tid >= o ? part[tid - o] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  int run = part[tid] - s;
  for (int u = u0; u < u1; ++u) { const int c = cur[u]; offsets[u] = run; cur[u] = run; run += c; }
  if (tid == 1023) offsets[U] = part[1023];
  __syncthreads();
  for (int base = 0; base < N; base += 1024) {
    const int i = base + tid, n = min(1024, N - base);
    const int key = i < N ? kv_index[i] : -1;
    keys[tid] = key;
    __syncthreads();
    int rank = 0;
    bool last = true;
    if (i < N) {
      for (int j = 0; j < n; ++j)
        if (keys[j] == key) { if (j < tid) ++rank; else if (j > tid) last = false; }
      order[cur[key] + rank] = i;
    }
    __syncthreads();
    if (i < N && last) cur[key] += rank + 1;
    __syncthreads();
  }
}

extern "C" {

int vqa_attention_fwd(int dtype, const void* q, const void* k, const void* v, int ldq, int ldk, int ldv, const float* kmask, float* probs,
                      void* ctx, int ldc, int B, int H, int Lq, int Lk, int hd, float p, unsigned long long seed, hipStream_t st) {
  return attention_fwd_valu(dtype, q, k, v, ldq, ldk, ldv, kmask, probs, ctx, ldc, B, H, Lq, Lk, hd, p, seed, nullptr, 0, st);
}
int vqa_attention_fwd_idx(int dtype, const void* q, const void* k, const void* v, int ldq, int ldk, int ldv, const int* kv_index, int n_kv,
                          const float* kmask, float* probs, void* ctx, int ldc, int B, int H, int Lq, int Lk, int hd, hipStream_t st) {
  if (!kv_index || n_kv < 0) return VQA_EARG;
  return attention_fwd_valu(dtype, q, k, v, ldq, ldk, ldv, kmask, probs, ctx, ldc, B, H, Lq, Lk, hd, 0.f, 0ull, kv_index, n_kv, st);
}
int vqa_attention_fwd_idx_train(int dtype, const void* q, const void* k, const void* v, int ldq, int ldk, int ldv, const int* kv_index,
                                int n_kv, const float* kmask, float* probs, void* ctx, int ldc, int B, int H, int Lq, int Lk, int hd,
                                float p, unsigned long long seed, hipStream_t st) {
  if (!kv_index || n_kv < 0 || !(p >= 0.f && p < 1.f)) return VQA_EARG;
  return attention_fwd_valu(dtype, q, k, v, ldq, ldk, ldv, kmask, probs, ctx, ldc, B, H, Lq, Lk, hd, p, seed, kv_index, n_kv, st);
}
int vqa_attention_fwd_mfma(const void* q, const void* k, const void* v, int ldq, int ldk, int ldv, const float* kmask, float* probs,
                           void* ctx, int ldc, int B, int H, int Lq, int Lk, int hd, float p, unsigned long long seed, hipStream_t st) {
  return attention_fwd_mfma(q, k, v, ldq, ldk, ldv, kmask, probs, ctx, ldc, B, H, Lq, Lk, hd, p, seed, nullptr, 0, st);
}
int vqa_attention_fwd_mfma_idx(const void* q, const void* k, const void* v, int ldq, int ldk, int ldv, const int* kv_index, int n_kv,
                               const float* kmask, float* probs, void* ctx, int ldc, int B, int H, int Lq, int Lk, int hd, hipStream_t st) {
  if (!kv_index || n_kv < 0) return VQA_EARG;
  return attention_fwd_mfma(q, k, v, ldq, ldk, ldv, kmask, probs, ctx, ldc, B, H, Lq, Lk, hd, 0.f, 0ull, kv_index, n_kv, st);
}
int vqa_attention_fwd_mfma_idx_train(const void* q, const void* k, const void* v, int ldq, int ldk, int ldv, const int* kv_index, int n_kv,
                                     const float* kmask, float* probs, void* ctx, int ldc, int B, int H, int Lq, int Lk, int hd, float p,
                                     unsigned long long seed, hipStream_t st) {
  if (!kv_index || n_kv < 0 || !(p >= 0.f && p < 1.f)) return VQA_EARG;
  return attention_fwd_mfma(q, k, v, ldq, ldk, ldv, kmask, probs, ctx, ldc, B, H, Lq, Lk, hd, p, seed, kv_index, n_kv, st);
}

int vqa_attention_bwd(int dtype, const void* dctx, int ldc, const void* q, const void* k, const void* v, int ldq, int ldk, int ldv,
                      const float* probs, void* dq, void* dk, void* dv, int lddq, int lddk, int lddv,
                      int B, int H, int Lq, int Lk, int hd, float p, unsigned long long seed, hipStream_t st) {
  if (!attn_bwd_valu_fits(Lq, Lk, hd)) return VQA_EARG;
  return attention_bwd_valu<false, 0>(dtype, dctx, ldc, q, k, v, ldq, ldk, ldv, probs, nullptr, nullptr, nullptr, 0, dq, dk, dv, lddq, lddk, lddv,
                                      B * H, H, Lq, Lk, hd, p, seed, st);
}
int vqa_attention_bwd_dp(int dtype, const void* dctx, int ldc, const void* q, const void* k, const void* v, int ldq, int ldk, int ldv,
                         const float* probs, const float* dprobs, void* dq, void* dk, void* dv, int lddq, int lddk, int lddv,
                         int B, int H, int Lq, int Lk, int hd, float p, unsigned long long seed, hipStream_t st) {
  if (!dprobs || !attn_bwd_valu_fits(Lq, Lk, hd)) return VQA_EARG;
  return attention_bwd_valu<true, 0>(dtype, dctx, ldc, q, k, v, ldq, ldk, ldv, probs, dprobs, nullptr, nullptr, 0, dq, dk, dv, lddq, lddk, lddv,
                                     B * H, H, Lq, Lk, hd, p, seed, st);
}
int vqa_attention_bwd_idx(int dtype, const void* dctx, int ldc, const void* q, const void* k, const void* v, int ldq, int ldk, int ldv,
                          const float* probs, const int* offsets, const int* order, int n_kv, void* dq, void* dk, void* dv,
                          int lddq, int lddk, int lddv, int B, int H, int Lq, int Lk, int hd, float p, unsigned long long seed,
                          hipStream_t st) {
  if (!dctx || !q || !k || !v || !probs || !offsets || (B > 0 && !order) || !dq || !dk || !dv || n_kv < 0 || B < 0 || H <= 0 ||
      Lq <= 0 || Lk <= 0 || hd <= 0 || !(p >= 0.f && p < 1.f))
    return VQA_EARG;
  const long long nkd = (long long)Lk * hd;
  if (!attn_bwd_valu_fits(Lq, Lk, hd) || nkd > 256 * 40) return VQA_EARG;
  if (n_kv == 0) return VQA_OK;
  return nkd <= 256 * 16
             ? attention_bwd_valu<false, 16>(dtype, dctx, ldc, q, k, v, ldq, ldk, ldv, probs, nullptr, offsets, order, B, dq, dk, dv, lddq, lddk,
                                             lddv, n_kv * H, H, Lq, Lk, hd, p, seed, st)
             : attention_bwd_valu<false, 40>(dtype, dctx, ldc, q, k, v, ldq, ldk, ldv, probs, nullptr, offsets, order, B, dq, dk, dv, lddq, lddk,
                                             lddv, n_kv * H, H, Lq, Lk, hd, p, seed, st);
}

int vqa_attention_bwd_mfma(const void* dctx, int ldc, const void* q, const void* k, const void* v, int ldq, int ldk, int ldv,
                           const float* probs, void* dq, void* dk, void* dv, int lddq, int lddk, int lddv,
                           int B, int H, int Lq, int Lk, int hd, float p, unsigned long long seed, hipStream_t st) {
  return attention_bwd_mfma_plain<false>(dctx, ldc, q, k, v, ldq, ldk, ldv, probs, nullptr, dq, dk, dv, lddq, lddk, lddv, B, H, Lq, Lk, hd, p, seed, st);
}
int vqa_attention_bwd_mfma_dp(const void* dctx, int ldc, const void* q, const void* k, const void* v, int ldq, int ldk, int ldv,
                              const float* probs, const float* dprobs, void* dq, void* dk, void* dv, int lddq, int lddk, int lddv,
                              int B, int H, int Lq, int Lk, int hd, float p, unsigned long long seed, hipStream_t st) {
  return attention_bwd_mfma_plain<true>(dctx, ldc, q, k, v, ldq, ldk, ldv, probs, dprobs, dq, dk, dv, lddq, lddk, lddv, B, H, Lq, Lk, hd, p, seed, st);
}
int vqa_attention_bwd_mfma_idx(const void* dctx, int ldc, const void* q, const void* k, const void* v, int ldq, int ldk, int ldv,
                               const float* probs, const int* offsets, const int* order, int n_kv, void* dq, void* dk, void* dv,
                               int lddq, int lddk, int lddv, int B, int H, int Lq, int Lk, int hd, float p, unsigned long long seed,
                               hipStream_t st) {
  if (!dctx || !q || !k || !v || !probs || !offsets || (B > 0 && !order) || !dq || !dk || !dv || n_kv < 0 || B < 0 || H <= 0 ||
      Lq <= 0 || Lq > 32 || Lk <= 0 || Lk > 160 || (hd != 32 && hd != 64) || (ldq % 8) || (ldk % 8) || (ldv % 8) || (ldc % 8) ||
      !(p >= 0.f && p < 1.f))
    return VQA_EARG;
  if (n_kv == 0) return VQA_OK;
  return attention_bwd_mfma<false, true>(dctx, ldc, q, k, v, ldq, ldk, ldv, probs, nullptr, offsets, order, B, dq, dk, dv, lddq, lddk, lddv,
                                         n_kv * H, H, Lq, Lk, hd, p, seed, st);
}

int vqa_index_csr(const int* kv_index, int N, int U, int* offsets, int* order, hipStream_t st) {
  if (N < 0 || U < 0 || U > 32768 || !offsets || (N > 0 && (!kv_index || !order))) return VQA_EARG;
  const size_t shm = (size_t)(U > 0 ? U : 1) * 4;
  (void)vqa_ensure_lds(reinterpret_cast<const void*>(&index_csr_kernel), shm);
  hipLaunchKernelGGL(index_csr_kernel, dim3(1), dim3(1024), shm, st, kv_index, N, U, offsets, order);
  VQA_LAUNCH_CHECK(); return VQA_OK;
}

}  // extern "C"
