// Token-side kernels for gfx950: embedding+positional encoding, LayerNorm, masked mean-pool, sigmoid gate, bias/ReLU/dropout
// backward, the fixed-order folds and the dtype casts.  (The optimizer tail -- L2 norm, clip, AdamW, weight EMA -- is optim_ops.hip;
// everything that reads the answer logits -- losses, metrics, answer scores, top-k -- is loss_ops.hip; multi-head attention is
// attention.hip.)
//   embedding*sqrt(d)+pe      models/text_encoder.py:504-510, :112-114
//   LayerNorm                 models/text_encoder.py:390,395,519 ; cross_attention.py:286-287,295 ; fusion.py:326
//   masked mean / gate        models/fusion.py:303-320, :160-166
// Rows are tokens ([B*L][D], D contiguous).  One 64-lane wave owns one row.
#include <cstdlib>
#include "common.h"

// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ void embed_fwd_kernel(const long long* __restrict__ ids, const float* __restrict__ emb, const float* __restrict__ pe,
                                 T* __restrict__ out, int rows, int L, int D, int V, float scale, float p, uint64_t seed) {
  seed = drop_resolve(seed);                        // (a flagged seed word names the step-state block: common.h)
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)rows * D) return;
  const int d = (int)(i % D), row = (int)(i / D), l = row % L;
  long long id = ids[row];
  float v = (id >= 0 && id < V) ? emb[(size_t)id * D + d] * scale : 0.f;
  v += pe[(size_t)l * D + d];
  if (p > 0.f) v = drop_keep32(drop_key(seed), (uint32_t)(i), p) ? v / (1.f - p) : 0.f;
  out[i] = from_f<T>(v);
}
// ---------------------------------------------------------------------------------------------------------------------------
// Fixed-order cross-workgroup reductions.  A kernel whose workgroups each hold a partial vector (bias / LayerNorm gamma, beta /
// position-embedding gradients, loss terms) stores it to its own row of a caller-provided scratch slab; fold_rows_kernel, launched
// right behind it on the same stream by the same C entry, sums the rows IN INDEX ORDER and performs the single += on the
// destination.  The result does not depend on the order the workgroups ran in (float atomics do): bit-reproducible gradients.
// (A same-kernel "last workgroup finishes" variant was measured first: its agent-scope release/acquire fences write back and
// invalidate the XCD's L2 once per workgroup, +50 us per LayerNorm backward; the kernel boundary gives the same visibility for
// one ~2 us launch.)
// block (64, 16): 64 columns x 16 row groups; a group sums a contiguous chunk of rows in index order with 16 loads in flight,
// the 16 group sums are folded in group order.  Columns [0, n0) go to dst0, [n0, ncols) to dst1.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void fold_rows_kernel(const float* __restrict__ part, int nrows, size_t stride, int ncols,
                                                         float* dst0, int n0, float* dst1) {
  const int c = blockIdx.x * 64 + threadIdx.x, rg = threadIdx.y;
  const int per = (nrows + 15) / 16, r0 = rg * per, r1 = min(nrows, r0 + per);
  float t = 0.f;
  if (c < ncols) {
    int r = r0;
    for (; r + 16 <= r1; r += 16) {
      float v[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) v[i] = part[(size_t)(r + i) * stride + c];
#pragma unroll
      for (int i = 0; i < 16; ++i) t += v[i];
    }
    for (; r < r1; ++r) t += part[(size_t)r * stride + c];
  }
  __shared__ float sh[16][64];
  sh[rg][threadIdx.x] = t;
  __syncthreads();
  if (rg == 0 && c < ncols) {
    float a = 0.f;
#pragma unroll
    for (int g = 0; g < 16; ++g) a += sh[g][threadIdx.x];
    if (c < n0) dst0[c] += a; else dst1[c - n0] += a;
  }
}
// (declared in common.h: loss_ops.hip folds its row terms through it, so the kernel's device code exists once)
void vqa_launch_fold(const float* part, int nrows, size_t stride, int ncols, float* dst0, int n0, float* dst1, hipStream_t st) {
  hipLaunchKernelGGL(fold_rows_kernel, dim3((ncols + 63) / 64), dim3(64, 16), 0, st, part, nrows, stride, ncols, dst0, n0, dst1);
}
// Many folds in one launch: the parameter gradients they produce are only read by the optimizer at the end of the step, so the engine
// queues them (defer_fold = 1 in the producing entries) and folds a whole gradient segment at once instead of paying one tiny launch per
// LayerNorm / bias on the data-gradient chain.  Same arithmetic per job as fold_rows_kernel (same row groups, same fold order).
constexpr int FOLD_MAXJOBS = 48;
struct FoldJob { const float* part; float* dst0; float* dst1; int nrows, ncols, n0; unsigned stride; };
struct FoldGroup { FoldJob j[FOLD_MAXJOBS]; int blk0[FOLD_MAXJOBS + 1]; int n; };
__global__ __launch_bounds__(1024) void fold_group_kernel(FoldGroup g) {
  int lo = 0, hi = g.n - 1;                                  // last job whose first block <= blockIdx.x (uniform)
  while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (g.blk0[mid] <= (int)blockIdx.x) lo = mid; else hi = mid - 1; }
  const FoldJob& job = g.j[lo];
  const float* __restrict__ part = job.part;
  const int nrows = job.nrows, ncols = job.ncols;
  const size_t stride = job.stride;
  const int c = ((int)blockIdx.x - g.blk0[lo]) * 64 + threadIdx.x, rg = threadIdx.y;
  const int per = (nrows + 15) / 16, r0 = rg * per, r1 = min(nrows, r0 + per);
  float t = 0.f;
  if (c < ncols) {
    int r = r0;
    for (; r + 16 <= r1; r += 16) {
      float v[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) v[i] = part[(size_t)(r + i) * stride + c];
#pragma unroll
      for (int i = 0; i < 16; ++i) t += v[i];
    }
    for (; r < r1; ++r) t += part[(size_t)r * stride + c];
  }
  __shared__ float sh[16][64];
  sh[rg][threadIdx.x] = t;
  __syncthreads();
  if (rg == 0 && c < ncols) {
    float a = 0.f;
#pragma unroll
    for (int q = 0; q < 16; ++q) a += sh[q][threadIdx.x];
    if (c < job.n0) job.dst0[c] += a; else job.dst1[c - job.n0] += a;
  }
}

// Gradient of the embedding table WITHOUT atomics: a workgroup owns 16 consecutive table rows, walks the id list in row order
// (1024 ids per pass, hits compacted in order through LDS) and adds the matching rows of dout to LDS accumulators in that order
// -> bit-reproducible, one writer per table element.  (The id list is rows*8 bytes, L2-resident, read V/16 times; the reference's
// nn.Embedding backward is a deterministic CPU scatter-add.)
constexpr int EMB_VB = 16;
template <typename T>
__global__ __launch_bounds__(256) void embed_bwd_kernel(const long long* __restrict__ ids, const T* __restrict__ dout, float* demb,
                                                        int rows, int D, int V, float scale, float p, uint64_t seed) {
  seed = drop_resolve(seed);                        // (a flagged seed word names the step-state block: common.h)
  extern __shared__ float eacc[];                             // [EMB_VB][D]
  __shared__ int list[1024];                                  // (row << 4) | (id - v0), in row order
  __shared__ int wcnt[4];
  const long long v0 = (long long)blockIdx.x * EMB_VB;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < EMB_VB * D; i += 256) eacc[i] = 0.f;
  const uint32_t dkey = drop_key(seed);
  const float ks = p > 0.f ? 1.f / (1.f - p) : 1.f;
  bool any = false;
  for (int base = 0; base < rows; base += 1024) {
    // thread t owns rows base + 4t .. base + 4t + 3 (row order == thread order, then k)
    int hit[4];
    int nh = 0;
    long long idv[4];
    const int rb = base + threadIdx.x * 4;
    if (rb + 3 < rows) {                                      // two 16-byte loads (ids is 8-byte aligned, rb is a multiple of 4)
      const u32x4 lo = *reinterpret_cast<const u32x4*>(ids + rb), hi = *reinterpret_cast<const u32x4*>(ids + rb + 2);
      idv[0] = (long long)(((unsigned long long)lo[1] << 32) | lo[0]); idv[1] = (long long)(((unsigned long long)lo[3] << 32) | lo[2]);
      idv[2] = (long long)(((unsigned long long)hi[1] << 32) | hi[0]); idv[3] = (long long)(((unsigned long long)hi[3] << 32) | hi[2]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) idv[k] = rb + k < rows ? ids[rb + k] : -1;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long long id = idv[k];
      const bool h = id >= v0 && id < v0 + EMB_VB && id > 0 && id < V;       // padding_idx = 0 receives no gradient
      hit[k] = h ? (int)(id - v0) : -1;
      nh += h;
    }
    // exclusive prefix of nh over the 256 threads: wave scan + wave totals through LDS
    int incl = nh;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(incl, o, 64); if (lane >= o) incl += u; }
    if (lane == 63) wcnt[wave] = incl;
    __syncthreads();
    int off = incl - nh, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) { if (w < wave) off += wcnt[w]; total += wcnt[w]; }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (hit[k] >= 0) list[off++] = ((base + threadIdx.x * 4 + k) << 4) | hit[k];
    __syncthreads();
    for (int i0 = 0; i0 < total; i0 += 8) {                   // 8 matching rows in flight, added in list order
      for (int d = threadIdx.x; d < D; d += 256) {
        float gq[8]; int sl[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int e = list[i0 + u < total ? i0 + u : total - 1], row = e >> 4;
          sl[u] = i0 + u < total ? (e & 15) : -1;
          const size_t o = (size_t)row * D + d;
          float g = to_f<T>(dout[o]) * scale;
          if (p > 0.f) g = drop_keep32(dkey, (uint32_t)o, p) ? g * ks : 0.f;
          gq[u] = g;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
          if (sl[u] >= 0) eacc[sl[u] * D + d] += gq[u];      // column d is only ever touched by this thread
      }
    }
    any |= total > 0;
    __syncthreads();
  }
  if (!any) return;
  for (int i = threadIdx.x; i < EMB_VB * D; i += 256) {
    const long long v = v0 + i / D;
    if (v > 0 && v < V && eacc[i] != 0.f) demb[(size_t)v * D + (i % D)] += eacc[i];
  }
}

// ---------------------------------------------------------------------------------------------
// LayerNorm: y = (x-mean)*rstd*gamma+beta ; optional dropout ; optional + addrow[row % period]
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void layernorm_fwd_kernel(const T* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            T* __restrict__ out, float* __restrict__ stats, int rows, int D, float eps,
                                                            float p, uint64_t seed, const float* __restrict__ addrow, int period) {
  seed = drop_resolve(seed);                        // (a flagged seed word names the step-state block: common.h)
  const int lane = threadIdx.x & 63;
  const int wid = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = (gridDim.x * blockDim.x) >> 6;
  for (int row = wid; row < rows; row += nw) {
    const T* xr = x + (size_t)row * D;
    float s = 0.f;
    for (int c = lane; c < D; c += 64) s += to_f<T>(xr[c]);
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
    for (int c = lane; c < D; c += 64) { const float t = to_f<T>(xr[c]) - mean; q += t * t; }
    const float rstd = rsqrtf(wave_sum(q) / (float)D + eps);
    if (lane == 0 && stats) { stats[row * 2] = mean; stats[row * 2 + 1] = rstd; }
    for (int c = lane; c < D; c += 64) {
      float y = (to_f<T>(xr[c]) - mean) * rstd * gamma[c] + beta[c];
      if (p > 0.f) y = drop_keep32(drop_key(seed), (uint32_t)((uint64_t)row * D + c), p) ? y / (1.f - p) : 0.f;
      if (addrow) y += addrow[(size_t)(row % period) * D + c];
      out[(size_t)row * D + c] = from_f<T>(y);
    }
  }
}

// bf16, D = 8 * LPR with LPR = 8 / 16 / 32 / 64 lanes per row: a lane owns one 16-byte segment of its row (one load, one store),
// 64 / LPR rows per wave; mean / variance are sub-wave shuffle reductions.  Same arithmetic as layernorm_fwd_kernel.
template <int LPR>
__global__ __launch_bounds__(256) void layernorm_fwd_bf16v_kernel(const bf16_t* __restrict__ x, const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta, bf16_t* __restrict__ out, float* __restrict__ stats,
                                                                  int rows, float eps, float p, uint64_t seed, const float* __restrict__ addrow, int period) {
  seed = drop_resolve(seed);                        // (a flagged seed word names the step-state block: common.h)
  constexpr int D = LPR * 8, RPW = 64 / LPR;
  const int lane = threadIdx.x & 63, sub = lane / LPR, sl = lane % LPR;
  const int wid = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = (gridDim.x * blockDim.x) >> 6;
  const int c0 = sl * 8;
  float gm[8], bt[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { gm[j] = gamma[c0 + j]; bt[j] = beta[c0 + j]; }
  const uint32_t dkey = drop_key(seed);
  const float ks = p > 0.f ? 1.f / (1.f - p) : 1.f;
  for (int r0 = wid * RPW; r0 < rows; r0 += nw * RPW) {
    const int row = r0 + sub;
    const bool live = row < rows;
    Vec16<bf16_t> v = live ? ldg16(x + (size_t)row * D + c0) : zero16<bf16_t>();
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) s += v.get(j);
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    const float mean = s / (float)D;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) { const float t = v.get(j) - mean; q += t * t; }
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
    const float rstd = rsqrtf(q / (float)D + eps);
    if (!live) continue;
    if (sl == 0 && stats) { stats[row * 2] = mean; stats[row * 2 + 1] = rstd; }
    Vec16<bf16_t> o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float y = (v.get(j) - mean) * rstd * gm[j] + bt[j];
      if (p > 0.f) y = drop_keep32(dkey, (uint32_t)((uint64_t)row * D + c0 + j), p) ? y * ks : 0.f;
      if (addrow) y += addrow[(size_t)(row % period) * D + c0 + j];
      o.set(j, y);
    }
    stg16(out + (size_t)row * D + c0, o);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const T* __restrict__ dout, const T* __restrict__ x, const float* __restrict__ gamma,
                                                            const float* __restrict__ stats, const T* __restrict__ addend, T* __restrict__ dx,
                                                            float* dgamma, float* dbeta, int rows, int D, float p, uint64_t seed,
                                                            float* dadd, int period, float* part) {
  seed = drop_resolve(seed);                        // (a flagged seed word names the step-state block: common.h)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wid = blockIdx.x * 4 + wave, nw = gridDim.x * 4;
  float ag[8], ab[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) ag[t] = ab[t] = 0.f;
  for (int row = wid; row < rows; row += nw) {
    const float mean = stats[row * 2], rstd = stats[row * 2 + 1];
    float gv[8], xh[8];
    float m1 = 0.f, m2 = 0.f;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int c = lane + 64 * t;
      gv[t] = 0.f; xh[t] = 0.f;
      if (c < D) {
        const size_t o = (size_t)row * D + c;
        float g = to_f<T>(dout[o]);
        if (dadd) atomicAdd(dadd + (size_t)(row % period) * D + c, g);
        if (p > 0.f) g = drop_keep32(drop_key(seed), (uint32_t)(o), p) ? g / (1.f - p) : 0.f;
        const float h = (to_f<T>(x[o]) - mean) * rstd;
        gv[t] = g; xh[t] = h;
        ag[t] += g * h; ab[t] += g;
        const float gy = g * gamma[c];
        m1 += gy; m2 += gy * h;
      }
    }
    m1 = wave_sum(m1) / (float)D; m2 = wave_sum(m2) / (float)D;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int c = lane + 64 * t;
      if (c < D) {
        const size_t o = (size_t)row * D + c;
        float r = rstd * (gv[t] * gamma[c] - m1 - xh[t] * m2);
        if (addend) r += to_f<T>(addend[o]);
        dx[o] = from_f<T>(r);
      }
    }
  }
  __shared__ float sh[2][4][512];
#pragma unroll
  for (int t = 0; t < 8; ++t) { sh[0][wave][lane + 64 * t] = ag[t]; sh[1][wave][lane + 64 * t] = ab[t]; }
  __syncthreads();
  if (!part) {                                                // no scratch: float atomics (order-dependent rounding)
    for (int c = threadIdx.x; c < D; c += 256) {
      atomicAdd(dgamma + c, sh[0][0][c] + sh[0][1][c] + sh[0][2][c] + sh[0][3][c]);
      atomicAdd(dbeta + c, sh[1][0][c] + sh[1][1][c] + sh[1][2][c] + sh[1][3][c]);
    }
    return;
  }
  for (int c = threadIdx.x; c < D; c += 256) {
    part[((size_t)blockIdx.x * 2) * D + c] = sh[0][0][c] + sh[0][1][c] + sh[0][2][c] + sh[0][3][c];
    part[((size_t)blockIdx.x * 2 + 1) * D + c] = sh[1][0][c] + sh[1][1][c] + sh[1][2][c] + sh[1][3][c];
  }
}

// out[n] += sum_b x[b][n] for x [B][N] (N % Vec16<T>::N == 0): the gradient of a row-periodic addend (position embedding),
// one 16-byte column group per thread, grid.y slices of the batch, one atomic per column per slice.
template <typename T>
__global__ __launch_bounds__(256) void colsum_rows_kernel(const T* __restrict__ x, float* out, int B, size_t N, float* part) {
  constexpr int VEC = Vec16<T>::N;
  const size_t n0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * VEC;
  const bool live = n0 < N;
  float acc[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) acc[j] = 0.f;
  if (live) {
#pragma unroll 4
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
      const Vec16<T> t = ldg16(x + (size_t)b * N + n0);
#pragma unroll
      for (int j = 0; j < VEC; ++j) acc[j] += t.get(j);
    }
  }
  if (!part) {                                                // no scratch: float atomics (order-dependent rounding)
    if (live) {
#pragma unroll
      for (int j = 0; j < VEC; ++j) atomicAdd(out + n0 + j, acc[j]);
    }
    return;
  }
  if (live) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) part[(size_t)blockIdx.y * N + n0 + j] = acc[j];
  }
}

// bf16, D % 8 == 0, D <= 512: lane owns channels [8*lane, 8*lane+8) -> one 16-byte load per operand per row, gamma and the
// dgamma/dbeta partial sums stay in registers, 8 waves per workgroup are reduced in LDS before the (few) atomics.
__global__ __launch_bounds__(512) void layernorm_bwd_bf16v_kernel(const bf16_t* __restrict__ dout, const bf16_t* __restrict__ x,
                                                                  const float* __restrict__ gamma, const float* __restrict__ stats,
                                                                  const bf16_t* __restrict__ addend, bf16_t* __restrict__ dx, float* dgamma,
                                                                  float* dbeta, int rows, int D, float p, uint64_t seed, float* dadd, int period,
                                                                  float* part) {
  seed = drop_resolve(seed);                        // (a flagged seed word names the step-state block: common.h)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wid = blockIdx.x * 8 + wave, nw = gridDim.x * 8;
  const int c0 = lane * 8;
  const bool act = c0 < D;
  float gm[8], ag[8], ab[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) { gm[t] = act ? gamma[c0 + t] : 0.f; ag[t] = 0.f; ab[t] = 0.f; }
  for (int row = wid; row < rows; row += nw) {
    const float mean = stats[row * 2], rstd = stats[row * 2 + 1];
    const size_t o = (size_t)row * D + c0;
    Vec16<bf16_t> dv = zero16<bf16_t>(), xv = zero16<bf16_t>(), av = zero16<bf16_t>();
    if (act) {
      dv = ldg16(dout + o); xv = ldg16(x + o);
      if (addend) av = ldg16(addend + o);
    }
    float gv[8], xh[8];
    float m1 = 0.f, m2 = 0.f;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      float g = dv.get(t);
      if (dadd && act) atomicAdd(dadd + (size_t)(row % period) * D + c0 + t, g);
      if (p > 0.f) g = drop_keep32(drop_key(seed), (uint32_t)(o + t), p) ? g / (1.f - p) : 0.f;
      const float h = act ? (xv.get(t) - mean) * rstd : 0.f;
      gv[t] = g; xh[t] = h;
      ag[t] += g * h; ab[t] += g;
      const float gy = g * gm[t];
      m1 += gy; m2 += gy * h;
    }
    m1 = wave_sum(m1) / (float)D; m2 = wave_sum(m2) / (float)D;
    if (act) {
      Vec16<bf16_t> ov;
#pragma unroll
      for (int t = 0; t < 8; ++t) ov.set(t, rstd * (gv[t] * gm[t] - m1 - xh[t] * m2) + av.get(t));
      stg16(dx + o, ov);
    }
  }
  __shared__ float sh[2][8][512];
#pragma unroll
  for (int t = 0; t < 8; ++t) { sh[0][wave][c0 + t] = ag[t]; sh[1][wave][c0 + t] = ab[t]; }
  __syncthreads();
  for (int c = threadIdx.x; c < D; c += 512) {
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int w = 0; w < 8; ++w) { a += sh[0][w][c]; b += sh[1][w][c]; }
    if (part) { part[((size_t)blockIdx.x * 2) * D + c] = a; part[((size_t)blockIdx.x * 2 + 1) * D + c] = b; }
    else { atomicAdd(dgamma + c, a); atomicAdd(dbeta + c, b); }
  }
}

// ---------------------------------------------------------------------------------------------
// masked mean over L:  out[b][col0+d] = sum_l x[b][l][d]*m[b][l] / max(sum_l m[b][l], 1)   (mask null -> plain mean)
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ void masked_pool_fwd_kernel(const T* __restrict__ x, const float* __restrict__ mask, T* __restrict__ out, int ldo, int col0, int L, int D) {
  const int b = blockIdx.x;
  float cnt = 0.f;
  for (int l = 0; l < L; ++l) cnt += mask ? mask[b * L + l] : 1.f;
  cnt = fmaxf(cnt, 1.f);
  for (int d = threadIdx.x; d < D; d += blockDim.x) {
    float s = 0.f;
    for (int l = 0; l < L; ++l) s += to_f<T>(x[((size_t)b * L + l) * D + d]) * (mask ? mask[b * L + l] : 1.f);
    out[(size_t)b * ldo + col0 + d] = from_f<T>(s / cnt);
  }
}
// dx[b][l][d] = (addend ? addend : 0) + dpool[b][col0+d]*m[b][l]/cnt
template <typename T>
__global__ void masked_pool_bwd_kernel(const T* __restrict__ dpool, int ldo, int col0, const float* __restrict__ mask, const T* __restrict__ addend,
                                       T* __restrict__ dx, int L, int D) {
  const int b = blockIdx.x;
  float cnt = 0.f;
  for (int l = 0; l < L; ++l) cnt += mask ? mask[b * L + l] : 1.f;
  cnt = fmaxf(cnt, 1.f);
  for (int i = threadIdx.x; i < L * D; i += blockDim.x) {
    const int l = i / D, d = i - l * D;
    const size_t o = ((size_t)b * L + l) * D + d;
    float r = to_f<T>(dpool[(size_t)b * ldo + col0 + d]) * (mask ? mask[b * L + l] : 1.f) / cnt;
    if (addend) r += to_f<T>(addend[o]);
    dx[o] = from_f<T>(r);
  }
}

// Both masked means of the fusion tail in one launch (models/fusion.py:281-296: attended queries and text features pooled with the
// same mask into cat = [att | txt]): blockIdx.y picks the tensor; the arithmetic per element is masked_pool_fwd_kernel's.
template <typename T>
__global__ void masked_pool_pair_fwd_kernel(const T* __restrict__ x0, const T* __restrict__ x1, const float* __restrict__ mask, T* __restrict__ out,
                                            int L, int D) {
  const int b = blockIdx.x, which = blockIdx.y;
  const T* __restrict__ x = which ? x1 : x0;
  float cnt = 0.f;
  for (int l = 0; l < L; ++l) cnt += mask ? mask[b * L + l] : 1.f;
  cnt = fmaxf(cnt, 1.f);
  for (int d = threadIdx.x; d < D; d += blockDim.x) {
    float s = 0.f;
    for (int l = 0; l < L; ++l) s += to_f<T>(x[((size_t)b * L + l) * D + d]) * (mask ? mask[b * L + l] : 1.f);
    out[(size_t)b * 2 * D + which * D + d] = from_f<T>(s / cnt);
  }
}
// ... and both backward broadcasts: dx{0,1}[b][l][d] = dcat[b][{0,D}+d] * m[b][l] / cnt
template <typename T>
__global__ void masked_pool_pair_bwd_kernel(const T* __restrict__ dcat, const float* __restrict__ mask, T* __restrict__ dx0, T* __restrict__ dx1,
                                            int L, int D) {
  const int b = blockIdx.x, which = blockIdx.y;
  T* __restrict__ dx = which ? dx1 : dx0;
  float cnt = 0.f;
  for (int l = 0; l < L; ++l) cnt += mask ? mask[b * L + l] : 1.f;
  cnt = fmaxf(cnt, 1.f);
  for (int d = threadIdx.x; d < D; d += blockDim.x) {
    const float g = to_f<T>(dcat[(size_t)b * 2 * D + which * D + d]);
    for (int l = 0; l < L; ++l)
      dx[((size_t)b * L + l) * D + d] = from_f<T>(g * (mask ? mask[b * L + l] : 1.f) / cnt);
  }
}

// gate: g = sigmoid(z); fused = g*att + (1-g)*txt, cat = [att | txt]  (models/fusion.py:160-166)
template <typename T>
__global__ void gate_fwd_kernel(const T* __restrict__ z, const T* __restrict__ cat, T* __restrict__ fused, int B, int D) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * D) return;
  const int b = i / D, d = i - b * D;
  const float g = 1.f / (1.f + expf(-to_f<T>(z[i])));
  const float a = to_f<T>(cat[(size_t)b * 2 * D + d]), t = to_f<T>(cat[(size_t)b * 2 * D + D + d]);
  fused[i] = from_f<T>(g * a + (1.f - g) * t);
}
template <typename T>
__global__ void gate_bwd_kernel(const T* __restrict__ dfused, const T* __restrict__ z, const T* __restrict__ cat, T* __restrict__ dz,
                                T* __restrict__ dcat, int B, int D) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * D) return;
  const int b = i / D, d = i - b * D;
  const float g = 1.f / (1.f + expf(-to_f<T>(z[i])));
  const float a = to_f<T>(cat[(size_t)b * 2 * D + d]), t = to_f<T>(cat[(size_t)b * 2 * D + D + d]);
  const float df = to_f<T>(dfused[i]);
  dz[i] = from_f<T>(df * (a - t) * g * (1.f - g));
  dcat[(size_t)b * 2 * D + d] = from_f<T>(df * g);
  dcat[(size_t)b * 2 * D + D + d] = from_f<T>(df * (1.f - g));
}

// out = a + b (either may alias out)
template <typename T>
__global__ void add_kernel(const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = from_f<T>(to_f<T>(a[i]) + to_f<T>(b[i]));
}

// gradient taps (graph-connected aux outputs): an fp32 upstream gradient added into a compute-dtype gradient buffer.
//   rows:  acc[r*ld + c] += g[r*cols + c]                                   (row-major, row stride ld: e.g. one half of dcat)
//   nchw:  acc[(b*HW + s)*C + c] += g[(b*C + c)*HW + s], HW = ld, C = cols  (aux['image_features'] into the NHWC stage-4 gradient)
// The NCHW form transposes through a 64-channel x 32-position LDS tile: reads run along positions, writes along channels.
template <typename T>
__global__ void grad_tap_rows_kernel(const float* __restrict__ g, T* __restrict__ acc, int cols, int ld, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t r = i / cols, c = i - r * cols;
  T* a = acc + r * ld + c;
  *a = from_f<T>(to_f<T>(*a) + g[i]);
}
template <typename T>
__global__ __launch_bounds__(256) void grad_tap_nchw_kernel(const float* __restrict__ g, T* __restrict__ acc, int C, int HW) {
  __shared__ float tile[64][33];
  const int b = blockIdx.z, c0 = blockIdx.y * 64, s0 = blockIdx.x * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int cc = ty; cc < 64; cc += 8) {
    const int c = c0 + cc, sp = s0 + tx;
    tile[cc][tx] = (c < C && sp < HW) ? g[((size_t)b * C + c) * HW + sp] : 0.f;
  }
  __syncthreads();
  const int cl = threadIdx.x & 63, sl = threadIdx.x >> 6;
  for (int ss = sl; ss < 32; ss += 4) {
    const int sp = s0 + ss, c = c0 + cl;
    if (sp < HW && c < C) {
      T* a = acc + ((size_t)b * HW + sp) * C + c;
      *a = from_f<T>(to_f<T>(*a) + tile[cl][ss]);
    }
  }
}

// dz = dout * [out>0] * dropout-keep-scale ; dbias[n] += column sums of dz
template <typename T>
__global__ __launch_bounds__(256) void bias_act_bwd_kernel(const T* __restrict__ dout, const T* __restrict__ outact, T* __restrict__ dz,
                                                           float* dbias, int M, int N, int relu_drop, float p, uint64_t seed,
                                                           float* part) {
  seed = drop_resolve(seed);                        // (a flagged seed word names the step-state block: common.h)
  // block handles a strip of 64 columns x rows_per_block rows; thread (r = tid/64, c = tid%64)
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), rl = threadIdx.x >> 6;
  const int rows_per = (M + gridDim.y - 1) / gridDim.y;
  const int r0 = blockIdx.y * rows_per, r1 = min(M, r0 + rows_per);
  float s = 0.f;
  if (c < N)
    for (int r = r0 + rl; r < r1; r += 4) {
      const size_t o = (size_t)r * N + c;
      float g = to_f<T>(dout[o]);
      if (outact) { if (!(to_f<T>(outact[o]) > 0.f)) g = 0.f; else if (p > 0.f) g /= (1.f - p); }   // relu(+dropout): out>0 encodes both
      else if (p > 0.f) g = drop_keep32(drop_key(seed), (uint32_t)(o), p) ? g / (1.f - p) : 0.f;
      if (dz) dz[o] = from_f<T>(g);
      s += g;
    }
  __shared__ float sh[4][64];
  sh[rl][threadIdx.x & 63] = s;
  __syncthreads();
  (void)relu_drop;
  if (!dbias) return;
  const float tcol = sh[0][threadIdx.x & 63] + sh[1][threadIdx.x & 63] + sh[2][threadIdx.x & 63] + sh[3][threadIdx.x & 63];
  if (!part) { if (rl == 0 && c < N) atomicAdd(dbias + c, tcol); return; }
  if (rl == 0 && c < N) part[(size_t)blockIdx.y * N + c] = tcol;
}

// Vectorised form of bias_act_bwd_kernel for N % 8 == 0 (bf16) / N % 4 == 0 (fp32): a thread owns one 16-byte column group and
// walks the rows of its strip (the scalar kernel above issues 2-byte loads: 18 us per call on tensors a few MB large).
// dbias: per-thread partial sums, folded over the block's row lanes in LDS, one atomic per column per block.
template <typename T>
__global__ __launch_bounds__(256) void bias_act_bwd_vec_kernel(const T* __restrict__ dout, const T* __restrict__ outact, T* __restrict__ dz,
                                                               float* dbias, int M, int N, float p, uint64_t seed, int rows_per,
                                                               float* part) {
  seed = drop_resolve(seed);                        // (a flagged seed word names the step-state block: common.h)
  constexpr int VEC = Vec16<T>::N;
  const int cvs = N / VEC;                                   // column groups per row
  const int gpb = cvs < 256 ? cvs : 256;                     // column groups handled by one block (per blockIdx.x)
  const int lanes_r = 256 / gpb;                             // rows in flight per block pass
  const int cg = blockIdx.x * gpb + threadIdx.x % gpb, rl = threadIdx.x / gpb;
  const int r0 = blockIdx.y * rows_per, r1 = min(M, r0 + rows_per);
  float s[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) s[j] = 0.f;
  const float ks = p > 0.f ? 1.f / (1.f - p) : 1.f;
  const uint32_t dkey = drop_key(seed);
  if (cg < cvs && rl < lanes_r) {
#pragma unroll 2
    for (int r = r0 + rl; r < r1; r += lanes_r) {
      const size_t o = (size_t)r * N + (size_t)cg * VEC;
      Vec16<T> d = ldg16(dout + o), a, z;
      if (outact) a = ldg16(outact + o);
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        float g = d.get(j);
        if (outact) { if (!(a.get(j) > 0.f)) g = 0.f; else g *= ks; }          // relu(+dropout): out > 0 encodes both masks
        else if (p > 0.f) g = drop_keep32(dkey, (uint32_t)(o + j), p) ? g * ks : 0.f;
        z.set(j, g);
        s[j] += g;
      }
      if (dz) stg16(dz + o, z);
    }
  }
  if (!dbias) return;
  __shared__ float sh[256 * VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) sh[threadIdx.x * VEC + j] = s[j];
  __syncthreads();
  for (int c = threadIdx.x; c < gpb * VEC; c += 256) {
    const int gq = c / VEC, j = c - gq * VEC;
    float t = 0.f;
    for (int r = 0; r < lanes_r; ++r) t += sh[(r * gpb + gq) * VEC + j];
    const int col = (blockIdx.x * gpb + gq) * VEC + j;
    if (col < N) { if (part) part[(size_t)blockIdx.y * N + col] = t; else atomicAdd(dbias + col, t); }
  }
}

template <typename TI, typename TO>
__global__ void convert_kernel(const TI* __restrict__ in, TO* __restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = from_f<TO>(to_f<TI>(in[i]));
}

// ---------------------------------------------------------------------------------------------
static inline unsigned g1(size_t n) { return (unsigned)((n + 255) / 256); }

extern "C" {

int vqa_embed_fwd(int dtype, const long long* ids, const float* emb, const float* pe, void* out, int rows, int L, int D, int V,
                  float scale, float p, unsigned long long seed, hipStream_t st) {
  const size_t n = (size_t)rows * D;
  DT(hipLaunchKernelGGL(embed_fwd_kernel<float>, dim3(g1(n)), dim3(256), 0, st, ids, emb, pe, (float*)out, rows, L, D, V, scale, p, seed),
     hipLaunchKernelGGL(embed_fwd_kernel<bf16_t>, dim3(g1(n)), dim3(256), 0, st, ids, emb, pe, (bf16_t*)out, rows, L, D, V, scale, p, seed));
  VQA_LAUNCH_CHECK(); return VQA_OK;
}
int vqa_embed_bwd(int dtype, const long long* ids, const void* dout, float* demb, int rows, int D, int V, float scale, float p,
                  unsigned long long seed, hipStream_t st) {
  if (D > 2048 || rows <= 0 || rows >= (1 << 27) || V <= 0) return VQA_EARG;
  const size_t shm = (size_t)EMB_VB * D * 4;
  const dim3 grid((V + EMB_VB - 1) / EMB_VB);
  (void)vqa_ensure_lds(dtype ? reinterpret_cast<const void*>(&embed_bwd_kernel<bf16_t>) : reinterpret_cast<const void*>(&embed_bwd_kernel<float>), shm);
  DT(hipLaunchKernelGGL(embed_bwd_kernel<float>, grid, dim3(256), shm, st, ids, (const float*)dout, demb, rows, D, V, scale, p, seed),
     hipLaunchKernelGGL(embed_bwd_kernel<bf16_t>, grid, dim3(256), shm, st, ids, (const bf16_t*)dout, demb, rows, D, V, scale, p, seed));
  VQA_LAUNCH_CHECK(); return VQA_OK;
}
int vqa_layernorm_fwd(int dtype, const void* x, const float* gamma, const float* beta, void* out, float* stats, int rows, int D, float eps,
                      float p, unsigned long long seed, const float* addrow, int period, hipStream_t st) {
  if (D > 512 || rows <= 0) return VQA_EARG;
  if (dtype && (D == 64 || D == 128 || D == 256 || D == 512)) {
    const int rpw = 512 / D, waves = (rows + rpw - 1) / rpw;
    const int g = (waves + 3) / 4 > 2048 ? 2048 : (waves + 3) / 4;
#define LNV(L) hipLaunchKernelGGL(layernorm_fwd_bf16v_kernel<L>, dim3(g), dim3(256), 0, st, (const bf16_t*)x, gamma, beta, (bf16_t*)out, stats, rows, eps, p, seed, addrow, period)
    if (D == 64) LNV(8); else if (D == 128) LNV(16); else if (D == 256) LNV(32); else LNV(64);
#undef LNV
    VQA_LAUNCH_CHECK(); return VQA_OK;
  }
  const int grid = (rows + 3) / 4 > 2048 ? 2048 : (rows + 3) / 4;
  DT(hipLaunchKernelGGL(layernorm_fwd_kernel<float>, dim3(grid), dim3(256), 0, st, (const float*)x, gamma, beta, (float*)out, stats, rows, D, eps, p, seed, addrow, period),
     hipLaunchKernelGGL(layernorm_fwd_kernel<bf16_t>, dim3(grid), dim3(256), 0, st, (const bf16_t*)x, gamma, beta, (bf16_t*)out, stats, rows, D, eps, p, seed, addrow, period));
  VQA_LAUNCH_CHECK(); return VQA_OK;
}
// launch geometry of vqa_layernorm_bwd (shared with the scratch-size query)
struct LnBwdGeom { int nb; bool colsum; unsigned gx, gy; size_t N; };
static LnBwdGeom ln_bwd_geom(int dtype, int rows, int D, int period) {
  LnBwdGeom g = {0, false, 0, 0, 0};
  if (dtype && D % 8 == 0) {                                 // 8 waves per block, ~2 rows per wave (4+ rows left 10 240-row tensors latency-bound: 13 us for 15 MB)
    const int rpb = vqa_env_int("VQA_LN_BWD_ROWS", 16);
    g.nb = (rows + rpb - 1) / rpb; if (g.nb > 1024) g.nb = 1024;
  }
  else g.nb = (rows + 15) / 16 > 2048 ? 2048 : (rows + 15) / 16;
  if (period > 0 && rows % period == 0 && ((size_t)period * D) % (dtype ? 8 : 4) == 0) {
    const int Bb = rows / period;
    g.colsum = true; g.N = (size_t)period * D;
    g.gx = (unsigned)((g.N / (dtype ? 8 : 4) + 255) / 256); g.gy = Bb < 32 ? Bb : 32;
  }
  return g;
}
// Floats of the `ws` scratch of vqa_layernorm_bwd (per-workgroup partial rows, see fold_rows_kernel).  period = the addrow period
// when dadd is requested, else 0.
long long vqa_layernorm_bwd_ws(int dtype, int rows, int D, int period) {
  if (D > 512 || rows <= 0) return 0;
  const LnBwdGeom g = ln_bwd_geom(dtype, rows, D, period);
  return (long long)g.nb * 2 * D + (g.colsum ? (long long)g.gy * (long long)g.N : 0);
}
// ws: scratch of vqa_layernorm_bwd_ws floats -> dgamma / dbeta / dadd are summed in a fixed order (bit-reproducible);
// nullptr -> float atomics (same values up to rounding order).
// Fold descriptors of vqa_layernorm_bwd for a caller that defers the folds (defer_fold = 1): returns the number of folds (1, or 2 with a
// position-embedding sum) and writes 5 values per fold to out: {offset into ws (floats), rows, row stride, columns, n0}; fold 0 targets
// (dgamma | dbeta) split at column n0 = D, fold 1 targets dadd.
int vqa_layernorm_bwd_folds(int dtype, int rows, int D, int period, long long* out) {
  if (D > 512 || rows <= 0 || !out) return 0;
  const LnBwdGeom g = ln_bwd_geom(dtype, rows, D, period);
  out[0] = 0; out[1] = g.nb; out[2] = 2 * D; out[3] = 2 * D; out[4] = D;
  if (!g.colsum) return 1;
  out[5] = (long long)g.nb * 2 * D; out[6] = g.gy; out[7] = (long long)g.N; out[8] = (long long)g.N; out[9] = (long long)g.N;
  return 2;
}
int vqa_layernorm_bwd(int dtype, const void* dout, const void* x, const float* gamma, const float* stats, const void* addend, void* dx,
                      float* dgamma, float* dbeta, int rows, int D, float p, unsigned long long seed, float* dadd, int period,
                      float* ws, int defer_fold, hipStream_t st) {
  if (D > 512 || rows <= 0 || (defer_fold && !ws)) return VQA_EARG;
  const LnBwdGeom g = ln_bwd_geom(dtype, rows, D, dadd ? period : 0);
  float* part_ln = ws;
  float* part_cs = ws ? ws + (size_t)g.nb * 2 * D : nullptr;
  if (dadd && g.colsum) {
    // position-embedding gradient as its own column-sum pass (one read of dout) instead of rows*D atomics inside the LN kernel
    const int Bb = rows / period;
    dim3 grid(g.gx, g.gy);
    DT(hipLaunchKernelGGL(colsum_rows_kernel<float>, grid, dim3(256), 0, st, (const float*)dout, dadd, Bb, g.N, part_cs),
       hipLaunchKernelGGL(colsum_rows_kernel<bf16_t>, grid, dim3(256), 0, st, (const bf16_t*)dout, dadd, Bb, g.N, part_cs));
    if (part_cs && !defer_fold) vqa_launch_fold(part_cs, (int)g.gy, g.N, (int)g.N, dadd, (int)g.N, nullptr, st);
    dadd = nullptr;
  }
  if (dtype && D % 8 == 0) {                               // vectorised bf16 path, >= 4 rows per wave, at most one workgroup per CU
    hipLaunchKernelGGL(layernorm_bwd_bf16v_kernel, dim3(g.nb), dim3(512), 0, st, (const bf16_t*)dout, (const bf16_t*)x, gamma, stats,
                       (const bf16_t*)addend, (bf16_t*)dx, dgamma, dbeta, rows, D, p, seed, dadd, period, part_ln);
  } else {
    DT(hipLaunchKernelGGL(layernorm_bwd_kernel<float>, dim3(g.nb), dim3(256), 0, st, (const float*)dout, (const float*)x, gamma, stats, (const float*)addend, (float*)dx, dgamma, dbeta, rows, D, p, seed, dadd, period, part_ln),
       hipLaunchKernelGGL(layernorm_bwd_kernel<bf16_t>, dim3(g.nb), dim3(256), 0, st, (const bf16_t*)dout, (const bf16_t*)x, gamma, stats, (const bf16_t*)addend, (bf16_t*)dx, dgamma, dbeta, rows, D, p, seed, dadd, period, part_ln));
  }
  if (part_ln && !defer_fold) vqa_launch_fold(part_ln, g.nb, (size_t)2 * D, 2 * D, dgamma, D, dbeta, st);
  VQA_LAUNCH_CHECK(); return VQA_OK;
}
int vqa_masked_pool_fwd(int dtype, const void* x, const float* mask, void* out, int ldo, int col0, int B, int L, int D, hipStream_t st) {
  DT(hipLaunchKernelGGL(masked_pool_fwd_kernel<float>, dim3(B), dim3(256), 0, st, (const float*)x, mask, (float*)out, ldo, col0, L, D),
     hipLaunchKernelGGL(masked_pool_fwd_kernel<bf16_t>, dim3(B), dim3(256), 0, st, (const bf16_t*)x, mask, (bf16_t*)out, ldo, col0, L, D));
  VQA_LAUNCH_CHECK(); return VQA_OK;
}
int vqa_masked_pool_pair_fwd(int dtype, const void* x0, const void* x1, const float* mask, void* out, int B, int L, int D, hipStream_t st) {
  if (!x0 || !x1 || !out || B <= 0 || L <= 0 || D <= 0) return VQA_EARG;
  DT(hipLaunchKernelGGL(masked_pool_pair_fwd_kernel<float>, dim3(B, 2), dim3(256), 0, st, (const float*)x0, (const float*)x1, mask, (float*)out, L, D),
     hipLaunchKernelGGL(masked_pool_pair_fwd_kernel<bf16_t>, dim3(B, 2), dim3(256), 0, st, (const bf16_t*)x0, (const bf16_t*)x1, mask, (bf16_t*)out, L, D));
  VQA_LAUNCH_CHECK(); return VQA_OK;
}
int vqa_masked_pool_pair_bwd(int dtype, const void* dcat, const float* mask, void* dx0, void* dx1, int B, int L, int D, hipStream_t st) {
  if (!dcat || !dx0 || !dx1 || B <= 0 || L <= 0 || D <= 0) return VQA_EARG;
  DT(hipLaunchKernelGGL(masked_pool_pair_bwd_kernel<float>, dim3(B, 2), dim3(256), 0, st, (const float*)dcat, mask, (float*)dx0, (float*)dx1, L, D),
     hipLaunchKernelGGL(masked_pool_pair_bwd_kernel<bf16_t>, dim3(B, 2), dim3(256), 0, st, (const bf16_t*)dcat, mask, (bf16_t*)dx0, (bf16_t*)dx1, L, D));
  VQA_LAUNCH_CHECK(); return VQA_OK;
}
int vqa_masked_pool_bwd(int dtype, const void* dpool, int ldo, int col0, const float* mask, const void* addend, void* dx, int B, int L, int D, hipStream_t st) {
  DT(hipLaunchKernelGGL(masked_pool_bwd_kernel<float>, dim3(B), dim3(256), 0, st, (const float*)dpool, ldo, col0, mask, (const float*)addend, (float*)dx, L, D),
     hipLaunchKernelGGL(masked_pool_bwd_kernel<bf16_t>, dim3(B), dim3(256), 0, st, (const bf16_t*)dpool, ldo, col0, mask, (const bf16_t*)addend, (bf16_t*)dx, L, D));
  VQA_LAUNCH_CHECK(); return VQA_OK;
}
int vqa_gate_fwd(int dtype, const void* z, const void* cat, void* fused, int B, int D, hipStream_t st) {
  DT(hipLaunchKernelGGL(gate_fwd_kernel<float>, dim3(g1((size_t)B * D)), dim3(256), 0, st, (const float*)z, (const float*)cat, (float*)fused, B, D),
     hipLaunchKernelGGL(gate_fwd_kernel<bf16_t>, dim3(g1((size_t)B * D)), dim3(256), 0, st, (const bf16_t*)z, (const bf16_t*)cat, (bf16_t*)fused, B, D));
  VQA_LAUNCH_CHECK(); return VQA_OK;
}
int vqa_gate_bwd(int dtype, const void* dfused, const void* z, const void* cat, void* dz, void* dcat, int B, int D, hipStream_t st) {
  DT(hipLaunchKernelGGL(gate_bwd_kernel<float>, dim3(g1((size_t)B * D)), dim3(256), 0, st, (const float*)dfused, (const float*)z, (const float*)cat, (float*)dz, (float*)dcat, B, D),
     hipLaunchKernelGGL(gate_bwd_kernel<bf16_t>, dim3(g1((size_t)B * D)), dim3(256), 0, st, (const bf16_t*)dfused, (const bf16_t*)z, (const bf16_t*)cat, (bf16_t*)dz, (bf16_t*)dcat, B, D));
  VQA_LAUNCH_CHECK(); return VQA_OK;
}
int vqa_grad_tap_add(int dtype, const float* g, void* acc, int rows, int cols, int ld, int layout, hipStream_t st) {
  if (!g || !acc || rows < 0 || cols <= 0 || ld <= 0) return VQA_EARG;
  if (rows == 0) return VQA_OK;
  if (layout == 0) {
    if (ld < cols) return VQA_EARG;
    const size_t n = (size_t)rows * cols;
    DT(hipLaunchKernelGGL(grad_tap_rows_kernel<float>, dim3(g1(n)), dim3(256), 0, st, g, (float*)acc, cols, ld, n),
       hipLaunchKernelGGL(grad_tap_rows_kernel<bf16_t>, dim3(g1(n)), dim3(256), 0, st, g, (bf16_t*)acc, cols, ld, n));
  } else if (layout == 1) {
    if (rows % ld) return VQA_EARG;
    const int B = rows / ld;
    if (B > 65535) return VQA_EARG;
    const dim3 grid((unsigned)((ld + 31) / 32), (unsigned)((cols + 63) / 64), (unsigned)B);
    DT(hipLaunchKernelGGL(grad_tap_nchw_kernel<float>, grid, dim3(256), 0, st, g, (float*)acc, cols, ld),
       hipLaunchKernelGGL(grad_tap_nchw_kernel<bf16_t>, grid, dim3(256), 0, st, g, (bf16_t*)acc, cols, ld));
  } else {
    return VQA_EARG;
  }
  VQA_LAUNCH_CHECK(); return VQA_OK;
}
int vqa_add(int dtype, const void* a, const void* b, void* out, long long n, hipStream_t st) {
  DT(hipLaunchKernelGGL(add_kernel<float>, dim3(g1((size_t)n)), dim3(256), 0, st, (const float*)a, (const float*)b, (float*)out, (size_t)n),
     hipLaunchKernelGGL(add_kernel<bf16_t>, dim3(g1((size_t)n)), dim3(256), 0, st, (const bf16_t*)a, (const bf16_t*)b, (bf16_t*)out, (size_t)n));
  VQA_LAUNCH_CHECK(); return VQA_OK;
}
// outact != null: relu (and dropout folded into out>0); outact == null && p>0: dropout mask regenerated from (seed, index)
struct BiasBwdGeom { bool vec; int gpb, rows_per; dim3 grid; };
static BiasBwdGeom bias_bwd_geom(int dtype, int M, int N) {
  BiasBwdGeom g;
  const int VEC = dtype ? 8 : 4;
  g.vec = N % VEC == 0 && M > 0 && (256 % (N / VEC < 256 ? N / VEC : 256)) == 0;
  if (g.vec) {
    const int cvs = N / VEC, gpb = cvs < 256 ? cvs : 256, lanes_r = 256 / gpb;
    int gy = (M + 4 * lanes_r - 1) / (4 * lanes_r);          // ~4 row passes per block (16 left a 10 240-row tensor with 80 latency-bound
                                                             // workgroups: 14 us for 5 MB); <= 1024 blocks in y
    if (gy > 1024) gy = 1024;
    if (gy < 1) gy = 1;
    g.gpb = gpb; g.rows_per = (M + gy - 1) / gy;
    g.grid = dim3((cvs + gpb - 1) / gpb, (M + g.rows_per - 1) / g.rows_per);
  } else {
    int gy = (M + 127) / 128; if (gy > 256) gy = 256; if (gy < 1) gy = 1;
    g.gpb = 0; g.rows_per = 0; g.grid = dim3((N + 63) / 64, gy);
  }
  return g;
}
// Floats of the `ws` scratch of vqa_bias_act_bwd (one partial row of N column sums per workgroup row).
long long vqa_bias_act_bwd_ws(int dtype, int M, int N) {
  if (M <= 0 || N <= 0) return 0;
  const BiasBwdGeom g = bias_bwd_geom(dtype, M, N);
  return (long long)g.grid.y * N;
}
// ws: vqa_bias_act_bwd_ws floats -> dbias summed in a fixed order (bit-reproducible); nullptr -> float atomics on dbias.
// rows of the partial slab (= rows of the deferred fold {offset 0, rows, stride N, N columns, n0 = N} into dbias)
int vqa_bias_act_bwd_fold_rows(int dtype, int M, int N) {
  if (M <= 0 || N <= 0) return 0;
  return (int)bias_bwd_geom(dtype, M, N).grid.y;
}
int vqa_bias_act_bwd(int dtype, const void* dout, const void* outact, void* dz, float* dbias, int M, int N, float p, unsigned long long seed,
                     float* ws, int defer_fold, hipStream_t st) {
  if (M <= 0 || N <= 0 || (defer_fold && !ws)) return VQA_EARG;
  const BiasBwdGeom g = bias_bwd_geom(dtype, M, N);
  if (g.vec) {
    DT(hipLaunchKernelGGL(bias_act_bwd_vec_kernel<float>, g.grid, dim3(256), 0, st, (const float*)dout, (const float*)outact, (float*)dz, dbias, M, N, p, seed, g.rows_per, ws),
       hipLaunchKernelGGL(bias_act_bwd_vec_kernel<bf16_t>, g.grid, dim3(256), 0, st, (const bf16_t*)dout, (const bf16_t*)outact, (bf16_t*)dz, dbias, M, N, p, seed, g.rows_per, ws));
  } else {
    DT(hipLaunchKernelGGL(bias_act_bwd_kernel<float>, g.grid, dim3(256), 0, st, (const float*)dout, (const float*)outact, (float*)dz, dbias, M, N, 0, p, seed, ws),
       hipLaunchKernelGGL(bias_act_bwd_kernel<bf16_t>, g.grid, dim3(256), 0, st, (const bf16_t*)dout, (const bf16_t*)outact, (bf16_t*)dz, dbias, M, N, 0, p, seed, ws));
  }
  if (ws && dbias && !defer_fold) vqa_launch_fold(ws, (int)g.grid.y, (size_t)N, N, dbias, N, nullptr, st);
  VQA_LAUNCH_CHECK(); return VQA_OK;
}
// dst0_j[c] (c < n0_j) / dst1_j[c - n0_j] += sum over rows r < nrows_j of part_j[r * stride_j + c], rows in index order -- the deferred folds of
// any number of vqa_layernorm_bwd / vqa_bias_act_bwd calls (defer_fold = 1) in ceil(njobs / 48) launches.
int vqa_fold_group(int njobs, const float* const* part, const int* nrows, const long long* stride, const int* ncols, float* const* dst0,
                   const int* n0, float* const* dst1, hipStream_t st) {
  if (njobs <= 0 || !part || !nrows || !stride || !ncols || !dst0 || !n0 || !dst1) return VQA_EARG;
  for (int base = 0; base < njobs; base += FOLD_MAXJOBS) {
    FoldGroup g;
    g.n = njobs - base < FOLD_MAXJOBS ? njobs - base : FOLD_MAXJOBS;
    g.blk0[0] = 0;
    for (int q = 0; q < g.n; ++q) {
      const int j = base + q;
      if (!part[j] || !dst0[j] || nrows[j] <= 0 || ncols[j] <= 0 || stride[j] <= 0 || stride[j] > 0xffffffffll || (n0[j] < ncols[j] && !dst1[j]))
        return VQA_EARG;
      g.j[q] = FoldJob{part[j], dst0[j], dst1[j], nrows[j], ncols[j], n0[j], (unsigned)stride[j]};
      g.blk0[q + 1] = g.blk0[q] + (ncols[j] + 63) / 64;
    }
    hipLaunchKernelGGL(fold_group_kernel, dim3(g.blk0[g.n]), dim3(64, 16), 0, st, g);
  }
  VQA_LAUNCH_CHECK(); return VQA_OK;
}
// dtype_in / dtype_out: 0 = f32, 1 = bf16
int vqa_convert(int dtype_in, int dtype_out, const void* in, void* out, long long n, hipStream_t st) {
  const unsigned g = g1((size_t)n);
  if (!dtype_in && dtype_out) hipLaunchKernelGGL((convert_kernel<float, bf16_t>), dim3(g), dim3(256), 0, st, (const float*)in, (bf16_t*)out, (size_t)n);
  else if (dtype_in && !dtype_out) hipLaunchKernelGGL((convert_kernel<bf16_t, float>), dim3(g), dim3(256), 0, st, (const bf16_t*)in, (float*)out, (size_t)n);
  else if (!dtype_in) hipLaunchKernelGGL((convert_kernel<float, float>), dim3(g), dim3(256), 0, st, (const float*)in, (float*)out, (size_t)n);
  else hipLaunchKernelGGL((convert_kernel<bf16_t, bf16_t>), dim3(g), dim3(256), 0, st, (const bf16_t*)in, (bf16_t*)out, (size_t)n);
  VQA_LAUNCH_CHECK(); return VQA_OK;
}

}  // extern "C"
