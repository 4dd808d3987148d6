// HBM-bound CNN-side kernels for gfx950: the stem's fused BN+ReLU+MaxPool tail (it shares stem_route.h with stem_conv.hip),
// squeeze-excitation, spatial attention and the NHWC <-> NCHW converters.  Activations are NHWC with T = float | bf16,
// every per-channel statistic / coefficient is fp32, every global access is a 16-byte vector.
// (The residual blocks' BatchNorm -- statistics, apply, backward -- is csrc/batchnorm.hip.)
//   BatchNorm2d        models/cnn_backbone.py:351 (the stem's; nn.BatchNorm2d defaults)
//   ReLU + MaxPool     models/cnn_backbone.py:352-353
//   SEAttention        models/attention_modules.py:109-136
//   SpatialAttention   models/attention_modules.py:223-243
#include "common.h"
#include "stem_route.h"

// ---------------------------------------------------------------------------------------------
// Stem tail: BN + ReLU + MaxPool3x3/2 p1 fused (the 112x112 activation is never written)
// ---------------------------------------------------------------------------------------------
// A workgroup owns a tile of 4 output rows x 7 output pairs (14 columns) x all channel vectors: its 9 x 29 input pixels are
// fetched once per tile through the CU's caches (1.13x the tensor); a row-major walk over the outputs fetched every input row for
// two output rows from HBM (PMC: 1.5x).  A thread owns one channel vector of TWO horizontally adjacent outputs: their 3x3/2
// windows share a column, so 15 loads (BN + ReLU applied once each) serve 2 outputs; the argmax bytes leave as packed stores.
constexpr int SP_ROWS = 4, SP_PAIRS = 7;
template <typename T>
__global__ __launch_bounds__(256) void stem_pool_fwd_kernel(const T* __restrict__ y, const float* __restrict__ coef, T* __restrict__ out,
                                                            uint8_t* __restrict__ idx, int B, int H, int W, int C, int Ho, int Wo, int trows) {
  constexpr int VEC = Vec16<T>::N;
  const int cv = C / VEC, Wp = (Wo + 1) >> 1;
  const int tiles_x = (Wp + SP_PAIRS - 1) / SP_PAIRS, tiles_y = (Ho + trows - 1) / trows;
  const int per_row = SP_PAIRS * cv;                       // threads per output row of the tile (host: per_row * trows <= 256)
  const int ry = threadIdx.x / per_row, rem = threadIdx.x - ry * per_row;
  if (ry >= trows) return;
  const int pr = rem / cv, c0 = (rem - pr * cv) * VEC;
  int t = blockIdx.x;
  const int tx = t % tiles_x; t /= tiles_x; const int ty = t % tiles_y; const int b = t / tiles_y;
  const int oh = ty * trows + ry, owp = tx * SP_PAIRS + pr;
  if (oh >= Ho || owp >= Wp) return;
  float sc[VEC], sh[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) { sc[j] = coef[c0 + j]; sh[j] = coef[C + c0 + j]; }
  const int ow0 = owp * 2;
  const bool two = ow0 + 1 < Wo;
  float best[2][VEC]; int bi[2][VEC];
#pragma unroll
  for (int o = 0; o < 2; ++o)
#pragma unroll
    for (int j = 0; j < VEC; ++j) { best[o][j] = -INFINITY; bi[o][j] = 0; }
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int ih = oh * 2 - 1 + r;
    if (ih < 0 || ih >= H) continue;
    const T* yr = y + (((size_t)b * H + ih) * W) * C + c0;
#pragma unroll
    for (int s5 = 0; s5 < 5; ++s5) {                         // input columns 2*ow0 - 1 .. 2*ow0 + 3
      const int iw = ow0 * 2 - 1 + s5;
      if (iw < 0 || iw >= W) continue;
      const Vec16<T> yy = ldg16(yr + (size_t)iw * C);
      float a[VEC];
#pragma unroll
      for (int j = 0; j < VEC; ++j) { const float v = yy.get(j) * sc[j] + sh[j]; a[j] = v < 0.f ? 0.f : v; }
      if (s5 < 3) {
#pragma unroll
        for (int j = 0; j < VEC; ++j)
          if (a[j] > best[0][j] || a[j] != a[j]) { best[0][j] = a[j]; bi[0][j] = r * 3 + s5; }     // first max wins, NaN propagates (ATen max_pool2d)
      }
      if (s5 >= 2) {
#pragma unroll
        for (int j = 0; j < VEC; ++j)
          if (a[j] > best[1][j] || a[j] != a[j]) { best[1][j] = a[j]; bi[1][j] = r * 3 + s5 - 2; }
      }
    }
  }
#pragma unroll
  for (int o = 0; o < 2; ++o) {
    if (o == 1 && !two) break;
    const size_t e = ((((size_t)b * Ho + oh) * Wo + ow0 + o) * C + c0);
    Vec16<T> ov;
    uint32_t pk[VEC / 4];
#pragma unroll
    for (int q4 = 0; q4 < VEC / 4; ++q4) pk[q4] = 0u;
#pragma unroll
    for (int j = 0; j < VEC; ++j) { ov.set(j, best[o][j]); pk[j >> 2] |= (uint32_t)bi[o][j] << (8 * (j & 3)); }
    stg16(out + e, ov);
#pragma unroll
    for (int q4 = 0; q4 < VEC / 4; ++q4) reinterpret_cast<uint32_t*>(idx + e)[q4] = pk[q4];
  }
}

template <typename T>
__global__ void stem_bwd_apply_kernel(const T* __restrict__ dpool, const uint8_t* __restrict__ idx, const T* __restrict__ y,
                                      const float* __restrict__ coef, const float* __restrict__ bc, T* __restrict__ dy,
                                      int B, int H, int W, int C, int Ho, int Wo) {
  constexpr int VEC = Vec16<T>::N;
  const int cv = C / VEC;
  const size_t total = (size_t)B * H * W * cv;
  float g[VEC];
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int v = (int)(i % cv); size_t r = i / cv;
    const int w = (int)(r % W); size_t q = r / W; const int h = (int)(q % H); const int b = (int)(q / H);
    const int c0 = v * VEC;
    Vec16<T> yy = ldg16(y + i * VEC), o;
    float sc[VEC], sh[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) { sc[j] = coef[c0 + j]; sh[j] = coef[C + c0 + j]; }
    stem_route<T>(dpool, idx, yy, sc, sh, b, h, w, c0, C, Ho, Wo, g);
#pragma unroll
    for (int j = 0; j < VEC; ++j) o.set(j, bc[c0 + j] * g[j] + bc[C + c0 + j] * yy.get(j) + bc[2 * C + c0 + j]);
    stg16(dy + i * VEC, o);
  }
}

// ---------------------------------------------------------------------------------------------
// Squeeze-excitation.  One workgroup per sample.
// ---------------------------------------------------------------------------------------------
// se buffers (fp32): pooled[B][C], hidden[B][Cr], scale[B][C]
template <typename T>
__global__ __launch_bounds__(256) void se_pool_fc_kernel(const T* __restrict__ x, const float* __restrict__ w1, const float* __restrict__ w2,
                                                         float* __restrict__ pooled, float* __restrict__ hidden, float* __restrict__ scale,
                                                         int HW, int C, int Cr, const float* __restrict__ part, int chunks) {
  constexpr int VEC = Vec16<T>::N;
  extern __shared__ float sh[];            // [256*VEC] scratch, then pooled[C], hidden[Cr]
  const int b = blockIdx.x, cv = C / VEC, lanes_r = 256 / cv;
  const int myv = threadIdx.x % cv, myr = threadIdx.x / cv;
  float s[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) s[j] = 0.f;
  if (!part && myr < lanes_r) {
    const T* xb = x + (size_t)b * HW * C + myv * VEC;
    int p = myr;
    for (; p + 3 * lanes_r < HW; p += 4 * lanes_r) {                 // 4 independent 16-byte loads in flight per thread
      Vec16<T> v0 = ldg16(xb + (size_t)p * C), v1 = ldg16(xb + (size_t)(p + lanes_r) * C);
      Vec16<T> v2 = ldg16(xb + (size_t)(p + 2 * lanes_r) * C), v3 = ldg16(xb + (size_t)(p + 3 * lanes_r) * C);
#pragma unroll
      for (int j = 0; j < VEC; ++j) s[j] += (v0.get(j) + v1.get(j)) + (v2.get(j) + v3.get(j));
    }
    for (; p < HW; p += lanes_r) {
      Vec16<T> v = ldg16(xb + (size_t)p * C);
#pragma unroll
      for (int j = 0; j < VEC; ++j) s[j] += v.get(j);
    }
  }
#pragma unroll
  for (int j = 0; j < VEC; ++j) sh[threadIdx.x * VEC + j] = s[j];
  __syncthreads();
  float* pl = sh + 256 * VEC; float* hd = pl + C;
  for (int c = threadIdx.x; c < C; c += 256) {
    const int v = c / VEC, j = c - v * VEC;
    float t = 0.f;
    if (part) { for (int k = 0; k < chunks; ++k) t += part[((size_t)b * chunks + k) * C + c]; }    // column sums left by vqa_bn_apply_pool / vqa_bn_apply_acc (batchnorm.hip)
    else { for (int r = 0; r < lanes_r; ++r) t += sh[(r * cv + v) * VEC + j]; }
    t /= (float)HW;
    pl[c] = t; pooled[(size_t)b * C + c] = t;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int jr = wave; jr < Cr; jr += 4) {
    float t = 0.f;
    for (int c = lane; c < C; c += 64) t += w1[(size_t)jr * C + c] * pl[c];
    t = wave_sum(t);
    if (lane == 0) { t = fmaxf(t, 0.f); hd[jr] = t; hidden[(size_t)b * Cr + jr] = t; }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    float t = 0.f;
    for (int jr = 0; jr < Cr; ++jr) t += w2[(size_t)c * Cr + jr] * hd[jr];
    scale[(size_t)b * C + c] = 1.f / (1.f + expf(-t));
  }
}

// out = x * rowscale[b][c] * pixscale[b][hw]   (either scale may be null)
// A thread owns one channel vector (c0 fixed) and walks pixels with 32-bit indices; b = pix / HW is one multiply-shift
// (mul_hw = ceil(2^40 / HW)).  (The former flat-index form spent more time in 64-bit divisions than in memory traffic.)
template <typename T>
__global__ __launch_bounds__(256) void scale_kernel(const T* __restrict__ x, const float* __restrict__ chscale, const float* __restrict__ pixscale,
                                                    T* __restrict__ out, unsigned npix, int C, unsigned long long mul_hw) {
  constexpr int VEC = Vec16<T>::N;
  const int cv = C / VEC, lanes_r = 256 / cv, c0 = (threadIdx.x % cv) * VEC, myr = threadIdx.x / cv;
  for (unsigned pix = blockIdx.x * lanes_r + myr; pix < npix; pix += gridDim.x * lanes_r) {
    const size_t e = (size_t)pix * C + c0;
    Vec16<T> v = ldg16(x + e), o;
    const float ps = pixscale ? pixscale[pix] : 1.f;
    if (chscale) {
      const unsigned b = (unsigned)(((unsigned long long)pix * mul_hw) >> 40);
      const f32x4* cs = reinterpret_cast<const f32x4*>(chscale + (size_t)b * C + c0);
#pragma unroll
      for (int q4 = 0; q4 < VEC / 4; ++q4) {
        const f32x4 c4 = cs[q4];
#pragma unroll
        for (int j = 0; j < 4; ++j) o.set(q4 * 4 + j, v.get(q4 * 4 + j) * ps * c4[j]);
      }
    } else {
#pragma unroll
      for (int j = 0; j < VEC; ++j) o.set(j, v.get(j) * ps);
    }
    stg16(out + e, o);
  }
}

// dhs[jr] = [hidden[jr] > 0] * sum_c z2[c] * w2[c][jr] for one sample, by the whole workgroup (round 4, third session).  w2 is [C][Cr]:
// the first form gave a wave one jr and walked c across its lanes -- 64 different cache lines per load (stride Cr floats), 16 K line
// requests per workgroup at C = 512 / Cr = 32, which is what made the 7 x 7 x 512 stage's SE backward take 80 us for 157 MB.  Here
// consecutive lanes read consecutive jr (thread = (channel group g, jr), G <= 64 groups), the G partials per jr are folded in group
// order through LDS: one writer, fixed order (bit-reproducible).  part: >= NT floats of LDS free at this point; ends with a barrier.
// Cr > NT (se_reduction < C / NT, e.g. se_reduction = 1 on a small map where vqa_se_bwd picks 256 threads): no room for even one
// group of Cr threads, so a thread owns jr = tid, tid + NT, ... and sums all of c itself (G = 1, same order as the one-group fold).
__device__ __forceinline__ void se_fc2_bwd(const float* __restrict__ z2, const float* __restrict__ w2, const float* __restrict__ hidden_b,
                                           float* __restrict__ dhs, float* __restrict__ dh_b, float* __restrict__ part, int C, int Cr, int NT) {
  if (Cr > NT) {
    for (int jr = threadIdx.x; jr < Cr; jr += NT) {
      float t = 0.f;
      for (int c = 0; c < C; ++c) t += z2[c] * w2[(size_t)c * Cr + jr];
      t = hidden_b[jr] > 0.f ? t : 0.f;
      dhs[jr] = t; dh_b[jr] = t;
    }
    __syncthreads();
    return;
  }
  const int G = min(NT / Cr, 64);
  const int jr = threadIdx.x % Cr, g = threadIdx.x / Cr;
  if (g < G) {
    float t = 0.f;
    for (int c = g; c < C; c += G) t += z2[c] * w2[(size_t)c * Cr + jr];
    part[g * Cr + jr] = t;
  }
  __syncthreads();
  if (threadIdx.x < Cr) {
    float t = 0.f;
    for (int q = 0; q < G; ++q) t += part[q * Cr + threadIdx.x];
    t = hidden_b[threadIdx.x] > 0.f ? t : 0.f;
    dhs[threadIdx.x] = t; dh_b[threadIdx.x] = t;
  }
  __syncthreads();
}

// SE backward, per sample: ds[c] = sum_hw dout*x ; through sigmoid / fc2 / relu / fc1 -> dz2[B][C], dh[B][Cr], dpool[B][C]
template <typename T>
__global__ __launch_bounds__(1024) void se_bwd_reduce_kernel(const T* __restrict__ dout, const T* __restrict__ x, const float* __restrict__ w1,
                                                            const float* __restrict__ w2, const float* __restrict__ hidden,
                                                            const float* __restrict__ scale, float* __restrict__ dz2, float* __restrict__ dh,
                                                            float* __restrict__ dpool, int HW, int C, int Cr) {
  constexpr int VEC = Vec16<T>::N;
  extern __shared__ float sh[];
  const int NT = blockDim.x;                      // 256 ... 1024 threads per sample (vqa_se_bwd picks; both forms use the same count)
  const int b = blockIdx.x, cv = C / VEC, lanes_r = NT / cv;
  const int myv = threadIdx.x % cv, myr = threadIdx.x / cv;
  float s[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) s[j] = 0.f;
  if (myr < lanes_r) {
    const size_t base = (size_t)b * HW * C + myv * VEC;
    int p = myr;
    for (; p + lanes_r < HW; p += 2 * lanes_r) {                     // 2 pixels = 4 independent 16-byte loads in flight per thread
      const size_t o0 = base + (size_t)p * C, o1 = base + (size_t)(p + lanes_r) * C;
      Vec16<T> d0 = ldg16(dout + o0), v0 = ldg16(x + o0), d1 = ldg16(dout + o1), v1 = ldg16(x + o1);
#pragma unroll
      for (int j = 0; j < VEC; ++j) s[j] += d0.get(j) * v0.get(j) + d1.get(j) * v1.get(j);
    }
    for (; p < HW; p += lanes_r) {
      const size_t off = base + (size_t)p * C;
      Vec16<T> d = ldg16(dout + off), v = ldg16(x + off);
#pragma unroll
      for (int j = 0; j < VEC; ++j) s[j] += d.get(j) * v.get(j);
    }
  }
#pragma unroll
  for (int j = 0; j < VEC; ++j) sh[threadIdx.x * VEC + j] = s[j];
  __syncthreads();
  float* z2 = sh + NT * VEC; float* dhs = z2 + C;
  for (int c = threadIdx.x; c < C; c += NT) {
    const int v = c / VEC, j = c - v * VEC;
    float t = 0.f;
    for (int r = 0; r < lanes_r; ++r) t += sh[(r * cv + v) * VEC + j];
    const float sg = scale[(size_t)b * C + c];
    t *= sg * (1.f - sg);
    z2[c] = t; dz2[(size_t)b * C + c] = t;
  }
  __syncthreads();
  se_fc2_bwd(z2, w2, hidden + (size_t)b * Cr, dhs, dh + (size_t)b * Cr, sh, C, Cr, NT);
  for (int c = threadIdx.x; c < C; c += NT) {
    float t = 0.f;
    for (int jr = 0; jr < Cr; ++jr) t += dhs[jr] * w1[(size_t)jr * C + c];
    dpool[(size_t)b * C + c] = t;
  }
}

// dx = dout*scale[b][c] + dpool[b][c]/HW   (same thread / index scheme as scale_kernel)
// xmask != nullptr: dx is additionally multiplied by (xmask > 0).  xmask is the SE input = the post-ReLU output of the stage's
// last residual block, so the block's backward receives its gradient ALREADY masked by its ReLU and never re-reads that
// activation (BatchNorm-backward reduce + apply and the identity-path addend: three reads saved for one here).
// BNRED (bn_y != nullptr): dx is the (masked) gradient entering the last block's bn2, so the BatchNorm-backward column sums
// sum dx | sum dx*xhat(bn_y) over the pixels this workgroup stores go to bn_slab[blockIdx.x][3][C] (the layout
// vqa_bn_bwd_finalize reads) -- the standalone reduce pass over dx and y2 is not run (one read of the stage output saved).
template <typename T, bool BNRED>
__global__ __launch_bounds__(256) void se_bwd_apply_kernel(const T* __restrict__ dout, const float* __restrict__ scale, const float* __restrict__ dpool,
                                                           T* __restrict__ dx, unsigned npix, int HW, int C, unsigned long long mul_hw,
                                                           const T* __restrict__ xmask, const T* __restrict__ bn_y, const float* __restrict__ bn_coef,
                                                           float* __restrict__ bn_slab, unsigned long long* __restrict__ bn_facc) {
  constexpr int VEC = Vec16<T>::N;
  const float inv = 1.f / (float)HW;
  const int cv = C / VEC, lanes_r = 256 / cv, c0 = (threadIdx.x % cv) * VEC, myr = threadIdx.x / cv;
  float sg[BNRED ? VEC : 1], sx[BNRED ? VEC : 1], bmean[BNRED ? VEC : 1], binv[BNRED ? VEC : 1];
  if constexpr (BNRED) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) { sg[j] = sx[j] = 0.f; bmean[j] = bn_coef[2 * C + c0 + j]; binv[j] = bn_coef[3 * C + c0 + j]; }
  }
#pragma unroll 2
  for (unsigned pix = blockIdx.x * lanes_r + myr; pix < npix; pix += gridDim.x * lanes_r) {
    const size_t e = (size_t)pix * C + c0;
    const unsigned b = (unsigned)(((unsigned long long)pix * mul_hw) >> 40);
    const f32x4* sp = reinterpret_cast<const f32x4*>(scale + (size_t)b * C + c0);
    const f32x4* dp = reinterpret_cast<const f32x4*>(dpool + (size_t)b * C + c0);
    Vec16<T> d = ldg16(dout + e), o, xm, yy;
    if (xmask) xm = ldg16(xmask + e);
    if constexpr (BNRED) yy = ldg16(bn_y + e);
#pragma unroll
    for (int q4 = 0; q4 < VEC / 4; ++q4) {
      const f32x4 s4 = sp[q4], p4 = dp[q4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float v = fmaf(d.get(q4 * 4 + j), s4[j], p4[j] * inv);     // explicit: both instantiations round identically
        if (xmask && !(xm.get(q4 * 4 + j) > 0.f)) v = 0.f;
        o.set(q4 * 4 + j, v);
      }
    }
    stg16(dx + e, o);
    if constexpr (BNRED) {
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const float g = o.get(j);                      // the value as stored: what bn_bwd_apply will read back
        sg[j] += g; sx[j] += g * (yy.get(j) - bmean[j]) * binv[j];
      }
    }
  }
  if constexpr (BNRED) {
    __shared__ float shm[2 * 256 * VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) { shm[threadIdx.x * VEC + j] = sg[j]; shm[(256 + threadIdx.x) * VEC + j] = sx[j]; }
    __syncthreads();
    for (int o2 = threadIdx.x; o2 < 3 * C; o2 += 256) {
      const int k = o2 / C, c = o2 - k * C, v = c / VEC, j = c - v * VEC;
      float t = 0.f;
      if (k < 2) for (int r = 0; r < lanes_r; ++r) t += shm[(k * 256 + r * cv + v) * VEC + j];
      if (bn_facc) {
        const int R = acc_replicas(C);
        if (k < 2) acc_add_fixed(bn_facc, (size_t)R * 3 * C, ((size_t)(blockIdx.x % R) * 3 + k) * C + c, t);
      }
      else bn_slab[((size_t)blockIdx.x * 3 + k) * C + c] = t;
    }
  }
}

// SE backward in ONE pass structure: the workgroup that reduced sample b (phase 1 of se_bwd_reduce_kernel) applies it right away
// (phase 2 of se_bwd_apply_kernel), so the second read of dout / x of that sample (0.4 MB ... 50 KB each) comes from the caches it
// just filled (L2 / Infinity Cache) instead of from HBM after the whole batch has streamed through twice.  Same arithmetic in the
// same order per element as the two-launch form: dx is bit-identical.  BNRED as in se_bwd_apply_kernel (accumulator mode only).
// NREG > 0 (round 4, third session): a thread visits the SAME (pixel, channel group) elements in both phases, so the first NREG vectors
// of dout it reads in phase 1 stay in its registers (+ one bit per element for x > 0) and phase 2 neither re-reads dout nor x for them:
// 7 -> 5 tensor passes where everything fits (NREG = 4: all of a 7 x 7 x 512 sample, 4 of 7 vectors at 14 x 14 x 256, 4 of 13 / 25 at stages 2 / 1; more kept vectors spill).  Loads are issued unconditionally on
// clamped addresses (a load under a branch makes hipcc drain the queue in front of it), the arithmetic per element and its order are
// the NREG = 0 kernel's: bit-identical dx and sums.
// NLDS > 0: the next NLDS vectors are parked in LDS between the phases (16 bytes per thread and vector behind the scratch region;
// one workgroup per CU is resident anyway at these register counts): 10 of a thread's 13 / 25 vectors at stages 2 / 1.
// TAILM: phase 1 also leaves ONE BYTE of [x > 0] per re-read vector in LDS, so phase 2 re-reads dout only (x was read for its signs).
template <typename T, bool BNRED, int NREG = 0, int NLDS = 0, bool TAILM = false>
__global__ __launch_bounds__(1024) void se_bwd_fused_kernel(const T* __restrict__ dout, const T* __restrict__ x, const float* __restrict__ w1,
                                                           const float* __restrict__ w2, const float* __restrict__ hidden,
                                                           const float* __restrict__ scale, float* __restrict__ dz2, float* __restrict__ dh,
                                                           float* __restrict__ dpool, T* __restrict__ dx, int HW, int C, int Cr, int mask_out,
                                                           const T* __restrict__ bn_y, const float* __restrict__ bn_coef,
                                                           unsigned long long* __restrict__ bn_facc) {
  constexpr int VEC = Vec16<T>::N;
  extern __shared__ float sh[];            // [NT*VEC] scratch | z2[C] | dhs[Cr] | dpl[C] | scl[C]
  const int NT = blockDim.x;               // 1024 threads per sample where the shape allows: one workgroup per sample is all the
                                           // parallelism there is (B = 512 samples on 256 CUs), and with 256 threads the two streaming
                                           // passes kept 8 waves per CU in flight: 3.3 TB/s against the 5 TB/s of the BatchNorm passes
  const int b = blockIdx.x, cv = C / VEC, lanes_r = NT / cv;
  const int myv = threadIdx.x % cv, myr = threadIdx.x / cv, c0 = myv * VEC;
  const size_t base = (size_t)b * HW * C + c0;
  float s[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) s[j] = 0.f;
  constexpr int NKEEP = NREG + NLDS;
  Vec16<T> dreg[NREG > 0 ? NREG : 1];
  unsigned mbits[NREG > 0 ? (NREG + 3) / 4 : 1];          // [x > 0] of the vectors kept in registers, 8 bits each
  u32x4* dl = reinterpret_cast<u32x4*>(sh + ((blockDim.x * VEC + 3 * C + Cr + 3) & ~3));      // [NLDS][NT] parked vectors ...
  unsigned char* dm = reinterpret_cast<unsigned char*>(dl + NLDS * blockDim.x);              // ... and their [x > 0] bytes
  unsigned char* dmt = dm + NLDS * blockDim.x;                                               // TAILM: [x > 0] bytes of the re-read vectors
  {
    int p = myr;
    if constexpr (NREG > 0) {
      static_assert(NREG % 2 == 0 && NLDS % 2 == 0 && VEC == 8, "kept vectors: pairs of 8-element vectors");
#pragma unroll
      for (int k = 0; k < (NREG + 3) / 4; ++k) mbits[k] = 0u;
#pragma unroll
      for (int i = 0; i < NREG; i += 2) {
        const int p0 = myr + i * lanes_r, p1 = p0 + lanes_r;
        const size_t o0 = base + (size_t)min(p0, HW - 1) * C, o1 = base + (size_t)min(p1, HW - 1) * C;
        Vec16<T> d0 = ldg16(dout + o0), v0 = ldg16(x + o0), d1 = ldg16(dout + o1), v1 = ldg16(x + o1);
        dreg[i] = d0; dreg[i + 1] = d1;
        unsigned m0 = 0u, m1 = 0u;
#pragma unroll
        for (int j = 0; j < VEC; ++j) { m0 |= (v0.get(j) > 0.f ? 1u : 0u) << j; m1 |= (v1.get(j) > 0.f ? 1u : 0u) << j; }
        mbits[i >> 2] |= m0 << ((i & 3) * 8);
        mbits[(i + 1) >> 2] |= m1 << (((i + 1) & 3) * 8);
        if (p1 < HW) {
#pragma unroll
          for (int j = 0; j < VEC; ++j) s[j] += d0.get(j) * v0.get(j) + d1.get(j) * v1.get(j);
        } else if (p0 < HW) {
#pragma unroll
          for (int j = 0; j < VEC; ++j) s[j] += d0.get(j) * v0.get(j);
        }
        // keep the PACKED vectors (4 registers each), not the 8 unpacked floats the products were formed from
        asm volatile("" : "+v"(dreg[i].raw), "+v"(dreg[i + 1].raw));
        if ((i & 2) != 0) __builtin_amdgcn_sched_barrier(0);     // two pairs of loads in flight at a time: hoisting all of them spills
      }
      if constexpr (NLDS > 0) {                                  // a rolled loop: unrolled, the parked vectors crowd the registers again
#pragma unroll 1
        for (int k = 0; k < NLDS; k += 2) {
          const int p0 = myr + (NREG + k) * lanes_r, p1 = p0 + lanes_r;
          const size_t o0 = base + (size_t)min(p0, HW - 1) * C, o1 = base + (size_t)min(p1, HW - 1) * C;
          Vec16<T> d0 = ldg16(dout + o0), v0 = ldg16(x + o0), d1 = ldg16(dout + o1), v1 = ldg16(x + o1);
          unsigned m0 = 0u, m1 = 0u;
#pragma unroll
          for (int j = 0; j < VEC; ++j) { m0 |= (v0.get(j) > 0.f ? 1u : 0u) << j; m1 |= (v1.get(j) > 0.f ? 1u : 0u) << j; }
          dl[k * blockDim.x + threadIdx.x] = d0.raw; dl[(k + 1) * blockDim.x + threadIdx.x] = d1.raw;
          dm[k * blockDim.x + threadIdx.x] = (unsigned char)m0; dm[(k + 1) * blockDim.x + threadIdx.x] = (unsigned char)m1;
          if (p1 < HW) {
#pragma unroll
            for (int j = 0; j < VEC; ++j) s[j] += d0.get(j) * v0.get(j) + d1.get(j) * v1.get(j);
          } else if (p0 < HW) {
#pragma unroll
            for (int j = 0; j < VEC; ++j) s[j] += d0.get(j) * v0.get(j);
          }
        }
      }
      p = myr + NKEEP * lanes_r;
    }
    int q = 0;
    for (; p + lanes_r < HW; p += 2 * lanes_r) {
      const size_t o0 = base + (size_t)p * C, o1 = base + (size_t)(p + lanes_r) * C;
      Vec16<T> d0 = ldg16(dout + o0), v0 = ldg16(x + o0), d1 = ldg16(dout + o1), v1 = ldg16(x + o1);
#pragma unroll
      for (int j = 0; j < VEC; ++j) s[j] += d0.get(j) * v0.get(j) + d1.get(j) * v1.get(j);
      if constexpr (TAILM) {
        unsigned m0 = 0u, m1 = 0u;
#pragma unroll
        for (int j = 0; j < VEC; ++j) { m0 |= (v0.get(j) > 0.f ? 1u : 0u) << j; m1 |= (v1.get(j) > 0.f ? 1u : 0u) << j; }
        dmt[q * blockDim.x + threadIdx.x] = (unsigned char)m0; dmt[(q + 1) * blockDim.x + threadIdx.x] = (unsigned char)m1;
        q += 2;
      }
    }
    for (; p < HW; p += lanes_r) {
      const size_t off = base + (size_t)p * C;
      Vec16<T> d = ldg16(dout + off), v = ldg16(x + off);
#pragma unroll
      for (int j = 0; j < VEC; ++j) s[j] += d.get(j) * v.get(j);
      if constexpr (TAILM) {
        unsigned m0 = 0u;
#pragma unroll
        for (int j = 0; j < VEC; ++j) m0 |= (v.get(j) > 0.f ? 1u : 0u) << j;
        dmt[q * blockDim.x + threadIdx.x] = (unsigned char)m0;
        q += 1;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < VEC; ++j) sh[threadIdx.x * VEC + j] = s[j];
  __syncthreads();
  float* z2 = sh + NT * VEC; float* dhs = z2 + C; float* dpl = dhs + Cr; float* scl = dpl + C;
  for (int c = threadIdx.x; c < C; c += NT) {
    const int v = c / VEC, j = c - v * VEC;
    float t = 0.f;
    for (int r = 0; r < lanes_r; ++r) t += sh[(r * cv + v) * VEC + j];
    const float sg = scale[(size_t)b * C + c];
    scl[c] = sg;
    t *= sg * (1.f - sg);
    z2[c] = t; dz2[(size_t)b * C + c] = t;
  }
  __syncthreads();
  se_fc2_bwd(z2, w2, hidden + (size_t)b * Cr, dhs, dh + (size_t)b * Cr, sh, C, Cr, NT);
  for (int c = threadIdx.x; c < C; c += NT) {
    float t = 0.f;
    for (int jr = 0; jr < Cr; ++jr) t += dhs[jr] * w1[(size_t)jr * C + c];
    dpl[c] = t; dpool[(size_t)b * C + c] = t;
  }
  __syncthreads();
  // ---- phase 2: dx = dout*scale + dpool/HW (* (x > 0)), this sample only
  const float inv = 1.f / (float)HW;
  float sc[VEC], dp[VEC], sg[BNRED ? VEC : 1], sx[BNRED ? VEC : 1], bmean[BNRED ? VEC : 1], binv[BNRED ? VEC : 1];
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    sc[j] = scl[c0 + j]; dp[j] = dpl[c0 + j] * inv;
    if (BNRED) { sg[j] = sx[j] = 0.f; bmean[j] = bn_coef[2 * C + c0 + j]; binv[j] = bn_coef[3 * C + c0 + j]; }
  }
  if constexpr (NREG > 0) {
#pragma unroll
    for (int i = 0; i < NREG; ++i) {
      const int p = myr + i * lanes_r;
      const size_t e = base + (size_t)min(p, HW - 1) * C;
      Vec16<T> o, yy;
      if constexpr (BNRED) yy = ldg16(bn_y + e);
      const unsigned mb = mbits[i >> 2] >> ((i & 3) * 8);
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        float v = fmaf(dreg[i].get(j), sc[j], dp[j]);
        if (mask_out && !((mb >> j) & 1u)) v = 0.f;
        o.set(j, v);
      }
      if (p < HW) {
        if constexpr (BNRED) {
#pragma unroll
          for (int j = 0; j < VEC; ++j) { const float g = o.get(j); sg[j] += g; sx[j] += g * (yy.get(j) - bmean[j]) * binv[j]; }
        }
        stg16(dx + e, o);
      }
      if ((i & 1) != 0) __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (NLDS > 0) {
#pragma unroll 2
      for (int k = 0; k < NLDS; ++k) {
        const int p = myr + (NREG + k) * lanes_r;
        if (p >= HW) break;
        const size_t e = base + (size_t)p * C;
        Vec16<T> o, yy, dk;
        if constexpr (BNRED) yy = ldg16(bn_y + e);
        dk.raw = dl[k * blockDim.x + threadIdx.x];               // (a thread reads back only what it wrote: no barrier needed)
        const unsigned mb = dm[k * blockDim.x + threadIdx.x];
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          float v = fmaf(dk.get(j), sc[j], dp[j]);
          if (mask_out && !((mb >> j) & 1u)) v = 0.f;
          o.set(j, v);
          if constexpr (BNRED) { const float g = o.get(j); sg[j] += g; sx[j] += g * (yy.get(j) - bmean[j]) * binv[j]; }
        }
        stg16(dx + e, o);
      }
    }
  }
  int qt = 0;
#pragma unroll 2
  for (int p = myr + NKEEP * lanes_r; p < HW; p += lanes_r) {
    const size_t e = base + (size_t)p * C;
    Vec16<T> d = ldg16(dout + e), o, xm, yy;
    unsigned mbt = 0xffu;
    if constexpr (TAILM) { mbt = dmt[qt * blockDim.x + threadIdx.x]; ++qt; }   // (TAILM is only dispatched with mask_out; own bytes: no barrier)
    else if (mask_out) xm = ldg16(x + e);
    if constexpr (BNRED) yy = ldg16(bn_y + e);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      float v = fmaf(d.get(j), sc[j], dp[j]);
      if (TAILM ? !((mbt >> j) & 1u) : (mask_out && !(xm.get(j) > 0.f))) v = 0.f;
      o.set(j, v);
      if constexpr (BNRED) { const float g = o.get(j); sg[j] += g; sx[j] += g * (yy.get(j) - bmean[j]) * binv[j]; }
    }
    stg16(dx + e, o);
  }
  if constexpr (BNRED) {
    __syncthreads();                         // everyone is done with the phase-1 scratch
#pragma unroll
    for (int j = 0; j < VEC; ++j) { sh[threadIdx.x * VEC + j] = sg[j]; }
    __syncthreads();
    const int R = acc_replicas(C);
    for (int c = threadIdx.x; c < C; c += NT) {
      const int v = c / VEC, j = c - v * VEC;
      float t = 0.f;
      for (int r = 0; r < lanes_r; ++r) t += sh[(r * cv + v) * VEC + j];
      acc_add_fixed(bn_facc, (size_t)R * 3 * C, ((size_t)(blockIdx.x % R) * 3 + 0) * C + c, t);
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < VEC; ++j) { sh[threadIdx.x * VEC + j] = sx[j]; }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += NT) {
      const int v = c / VEC, j = c - v * VEC;
      float t = 0.f;
      for (int r = 0; r < lanes_r; ++r) t += sh[(r * cv + v) * VEC + j];
      acc_add_fixed(bn_facc, (size_t)R * 3 * C, ((size_t)(blockIdx.x % R) * 3 + 1) * C + c, t);
    }
  }
}

// (Round 4: a SPLIT form -- per-chunk column sums over a (row chunk, sample) grid, then fold + FC backward + apply per workgroup --
// was built to give this pass more parallelism and measured SLOWER in isolation at every stage: 250 / 129 / 77 / 89 us against
// 222 / 110 / 69 / 85 us for this kernel at B = 512 (tools/bench_hbm_kernels.py).  The one-workgroup-per-sample kernel is not short of
// parallelism: it moves 6 tensor passes (r dout x | r dout x y2, w dx) at 5.5 TB/s; the "3.0 TB/s" of the bench line divides the FOUR
// algorithmic passes by its time, i.e. it prices the second read of dout / x as a cache hit, which 512 x 0.8 MB in flight are not.)
// dw2[c][j] += sum_b dz2[b][c]*hidden[b][j] ; dw1[j][c] += sum_b dh[b][j]*pooled[b][c]
// A workgroup owns 8 consecutive (j, c) pairs (c fastest) and splits the batch over 32 thread slices; the slices are folded in LDS
// in slice order, so every weight has ONE writer and a fixed summation order (bit-reproducible, no atomics, no scratch).
// OUTS = 32 (round 4, third session): a wave's load covers two full 128-byte rows of dz2 / pooled instead of eight 32-byte pieces
// (C * Cr = 16 384 outputs at the 512-channel stage: 28 -> ~10 us); same 32 slices, same fold order: the same bits as OUTS = 8.
template <int OUTS>
__global__ __launch_bounds__(OUTS * 32) void se_wgrad_kernel(const float* __restrict__ dz2, const float* __restrict__ hidden, const float* __restrict__ dh,
                                const float* __restrict__ pooled, float* dw1, float* dw2, int B, int C, int Cr) {
  const int pr = threadIdx.x % OUTS, q = threadIdx.x / OUTS;
  const int i = blockIdx.x * OUTS + pr;
  const bool live = i < C * Cr;
  const int j = live ? i / C : 0, c = live ? i - j * C : 0;
  float t2 = 0.f, t1 = 0.f;
  if (live) {
#pragma unroll 4
    for (int b = q; b < B; b += 32) {
      t2 += dz2[(size_t)b * C + c] * hidden[(size_t)b * Cr + j];
      t1 += dh[(size_t)b * Cr + j] * pooled[(size_t)b * C + c];
    }
  }
  __shared__ float sh[2][32][OUTS];
  sh[0][q][pr] = t2; sh[1][q][pr] = t1;
  __syncthreads();
  if (threadIdx.x < 2 * OUTS && blockIdx.x * OUTS + (threadIdx.x % OUTS) < C * Cr) {
    const int which = threadIdx.x / OUTS, pp = threadIdx.x % OUTS;
    const int ii = blockIdx.x * OUTS + pp, jj = ii / C, cc = ii - jj * C;
    float t = 0.f;
#pragma unroll
    for (int s_ = 0; s_ < 32; ++s_) t += sh[which][s_][pp];
    if (which == 0) dw2[(size_t)cc * Cr + jj] += t; else dw1[(size_t)jj * C + cc] += t;
  }
}
static void launch_se_wgrad(const float* dz2, const float* hidden, const float* dh, const float* pooled, float* dw1, float* dw2, int B, int C, int Cr,
                            hipStream_t st) {
  if (C * Cr >= 1024) hipLaunchKernelGGL(se_wgrad_kernel<32>, dim3((C * Cr + 31) / 32), dim3(1024), 0, st, dz2, hidden, dh, pooled, dw1, dw2, B, C, Cr);
  else hipLaunchKernelGGL(se_wgrad_kernel<8>, dim3((C * Cr + 7) / 8), dim3(256), 0, st, dz2, hidden, dh, pooled, dw1, dw2, B, C, Cr);
}

// ---------------------------------------------------------------------------------------------
// Spatial attention.  pooled2[B][H][W][2] fp32 (max, mean), amax[B][H][W] int (argmax channel), amap[B][H][W] fp32
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ void spatial_pool_kernel(const T* __restrict__ x, float* __restrict__ pooled2, int* __restrict__ amax, size_t npix, int C) {
  constexpr int VEC = Vec16<T>::N;
  const int lane = threadIdx.x & 63;
  const size_t wid = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = ((size_t)gridDim.x * blockDim.x) >> 6;
  for (size_t p = wid; p < npix; p += nw) {
    float mx = -INFINITY, sm = 0.f; int mi = 0x7fffffff;
    for (int c0 = lane * VEC; c0 < C; c0 += 64 * VEC) {
      Vec16<T> v = ldg16(x + p * C + c0);
#pragma unroll
      for (int j = 0; j < VEC; ++j) { const float f = v.get(j); sm += f; if (f > mx) { mx = f; mi = c0 + j; } }
    }
    sm = wave_sum(sm);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {      // max with lowest-index tie-break (torch.max picks the first maximum)
      const float om = __shfl_xor(mx, o, 64); const int oi = __shfl_xor(mi, o, 64);
      if (om > mx || (om == mx && oi < mi)) { mx = om; mi = oi; }
    }
    if (lane == 0) { pooled2[p * 2] = mx; pooled2[p * 2 + 1] = sm / (float)C; amax[p] = mi; }
  }
}

// amap = sigmoid(conv7x7(pooled2; w[2][7][7]))   (w is the (1,2,7,7) parameter, ch-major)
__global__ void spatial_conv_kernel(const float* __restrict__ pooled2, const float* __restrict__ w, float* __restrict__ amap, int B, int H, int W) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)B * H * W) return;
  const int ww = (int)(i % W); size_t q = i / W; const int h = (int)(q % H); const int b = (int)(q / H);
  float t = 0.f;
  for (int r = 0; r < 7; ++r) {
    const int ih = h + r - 3; if (ih < 0 || ih >= H) continue;
    for (int s = 0; s < 7; ++s) {
      const int iw = ww + s - 3; if (iw < 0 || iw >= W) continue;
      const float* pp = pooled2 + (((size_t)b * H + ih) * W + iw) * 2;
      t += pp[0] * w[r * 7 + s] + pp[1] * w[49 + r * 7 + s];
    }
  }
  amap[i] = 1.f / (1.f + expf(-t));
}

// dpre[p] = (sum_c dout*x) * a*(1-a)
template <typename T>
__global__ void spatial_bwd_reduce_kernel(const T* __restrict__ dout, const T* __restrict__ x, const float* __restrict__ amap,
                                          float* __restrict__ dpre, size_t npix, int C) {
  constexpr int VEC = Vec16<T>::N;
  const int lane = threadIdx.x & 63;
  const size_t wid = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nw = ((size_t)gridDim.x * blockDim.x) >> 6;
  for (size_t p = wid; p < npix; p += nw) {
    float s = 0.f;
    for (int c0 = lane * VEC; c0 < C; c0 += 64 * VEC) {
      Vec16<T> d = ldg16(dout + p * C + c0), v = ldg16(x + p * C + c0);
#pragma unroll
      for (int j = 0; j < VEC; ++j) s += d.get(j) * v.get(j);
    }
    s = wave_sum(s);
    if (lane == 0) { const float a = amap[p]; dpre[p] = s * a * (1.f - a); }
  }
}

// dpool2[b][h][w][ch] = sum_{r,s} dpre[b][h-r+3][w-s+3] * w[ch][r][s]
__global__ void spatial_bwd_conv_kernel(const float* __restrict__ dpre, const float* __restrict__ w, float* __restrict__ dpool2, int B, int H, int W) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)B * H * W) return;
  const int ww = (int)(i % W); size_t q = i / W; const int h = (int)(q % H); const int b = (int)(q / H);
  float t0 = 0.f, t1 = 0.f;
  for (int r = 0; r < 7; ++r) {
    const int oh = h - r + 3; if (oh < 0 || oh >= H) continue;
    for (int s = 0; s < 7; ++s) {
      const int ow = ww - s + 3; if (ow < 0 || ow >= W) continue;
      const float d = dpre[((size_t)b * H + oh) * W + ow];
      t0 += d * w[r * 7 + s]; t1 += d * w[49 + r * 7 + s];
    }
  }
  dpool2[i * 2] = t0; dpool2[i * 2 + 1] = t1;
}

// dx = dout*amap[p] + dpool2[p][1]/C + (c == amax[p]) * dpool2[p][0]
template <typename T>
__global__ void spatial_bwd_apply_kernel(const T* __restrict__ dout, const float* __restrict__ amap, const float* __restrict__ dpool2,
                                         const int* __restrict__ amax, T* __restrict__ dx, unsigned npix, int C) {
  constexpr int VEC = Vec16<T>::N;
  const float inv = 1.f / (float)C;
  const int cv = C / VEC, lanes_r = 256 / cv, c0 = (threadIdx.x % cv) * VEC, myr = threadIdx.x / cv;
  for (unsigned p = blockIdx.x * lanes_r + myr; p < npix; p += gridDim.x * lanes_r) {
    const size_t e = (size_t)p * C + c0;
    Vec16<T> d = ldg16(dout + e), o;
    const float a = amap[p], dm = dpool2[p * 2], da = dpool2[p * 2 + 1] * inv; const int mi = amax[p];
#pragma unroll
    for (int j = 0; j < VEC; ++j) o.set(j, d.get(j) * a + da + ((c0 + j) == mi ? dm : 0.f));
    stg16(dx + e, o);
  }
}

// part[y][ch][r][s] = sum over slice y of the pixels of dpre[b][h][w] * pooled2[b][h+r-3][w+s-3][ch] ; one block per ((ch,r,s), slice);
// spatial_wgrad_finish_kernel folds the slices in slice order into dw (one writer per weight: bit-reproducible, no atomics).
constexpr int SPATIAL_WG_SLICES = 16;
__global__ __launch_bounds__(256) void spatial_wgrad_kernel(const float* __restrict__ dpre, const float* __restrict__ pooled2, float* __restrict__ part, int B, int H, int W) {
  const int o = blockIdx.x, ch = o / 49, r = (o % 49) / 7, s = o % 7;
  float t = 0.f;
  const size_t n = (size_t)B * H * W;
  for (size_t i = (size_t)blockIdx.y * 256 + threadIdx.x; i < n; i += (size_t)gridDim.y * 256) {
    const int ww = (int)(i % W); size_t q = i / W; const int h = (int)(q % H); const int b = (int)(q / H);
    const int ih = h + r - 3, iw = ww + s - 3;
    if (ih < 0 || ih >= H || iw < 0 || iw >= W) continue;
    t += dpre[i] * pooled2[(((size_t)b * H + ih) * W + iw) * 2 + ch];
  }
  __shared__ float sh[4];
  t = wave_sum(t);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = t;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.y * 98 + o] = sh[0] + sh[1] + sh[2] + sh[3];
}
__global__ void spatial_wgrad_finish_kernel(const float* __restrict__ part, float* dw) {
  const int o = threadIdx.x;
  if (o >= 98) return;
  float t = 0.f;
#pragma unroll
  for (int y = 0; y < SPATIAL_WG_SLICES; ++y) t += part[y * 98 + o];
  dw[o] += t;
}

// NHWC(T) <-> NCHW(fp32) boundary conversions (aux['image_features'] is NCHW fp32 at the API boundary)
template <typename T>
__global__ void nhwc_to_nchw_kernel(const T* __restrict__ in, float* __restrict__ out, int B, int HW, int C) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)B * HW * C) return;
  const int p = (int)(i % HW); size_t q = i / HW; const int c = (int)(q % C); const size_t b = q / C;
  out[i] = to_f<T>(in[(b * HW + p) * C + c]);
}
template <typename T>
__global__ void nchw_to_nhwc_kernel(const float* __restrict__ in, T* __restrict__ out, int B, int HW, int C) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)B * HW * C) return;
  const int c = (int)(i % C); size_t q = i / C; const int p = (int)(q % HW); const size_t b = q / HW;
  out[i] = from_f<T>(in[(b * C + c) * HW + p]);
}

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
// grid for the pixel-walking elementwise kernels (a thread owns a channel vector): enough workgroups to cover the pixels, capped
static inline int px_grid(size_t npix, int C, int VEC) { const size_t lr = 256 / (C / VEC), g = (npix + lr - 1) / lr; return (int)(g > 16384 ? 16384 : (g ? g : 1)); }
static inline unsigned long long magic40(unsigned d) { return ((1ull << 40) + d - 1) / d; }   // (x * m) >> 40 == x / d for x*d < 2^40
static inline int ew_grid(size_t n) { size_t g = (n + 255) / 256; return (int)(g > 16384 ? 16384 : (g ? g : 1)); }

extern "C" {

int vqa_stem_pool_fwd(int dtype, const void* y, const float* coef, void* out, uint8_t* idx, int B, int H, int W, int C, hipStream_t st) {
  const int VEC = dtype ? 8 : 4, Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
  const int per_row = SP_PAIRS * (C / VEC);
  if (C % 8 || per_row > 256) return VQA_EARG;
  const int trows = 256 / per_row < SP_ROWS ? 256 / per_row : SP_ROWS;      // 4 rows (bf16, C = 64), 2 (fp32)
  const int Wp = (Wo + 1) / 2;
  const long long tiles = (long long)B * ((Ho + trows - 1) / trows) * ((Wp + SP_PAIRS - 1) / SP_PAIRS);
  if (tiles <= 0 || tiles > 0x7fffffffll) return VQA_EARG;
  const int threads = (per_row * trows + 63) / 64 * 64;
  DT(hipLaunchKernelGGL(stem_pool_fwd_kernel<float>, dim3((unsigned)tiles), dim3(threads), 0, st, (const float*)y, coef, (float*)out, idx, B, H, W, C, Ho, Wo, trows),
     hipLaunchKernelGGL(stem_pool_fwd_kernel<bf16_t>, dim3((unsigned)tiles), dim3(threads), 0, st, (const bf16_t*)y, coef, (bf16_t*)out, idx, B, H, W, C, Ho, Wo, trows));
  VQA_LAUNCH_CHECK(); return VQA_OK;
}
int vqa_stem_bwd_apply(int dtype, const void* dpool, const uint8_t* idx, const void* y, const float* coef, const float* bc, void* dy, int B, int H, int W, int C, hipStream_t st) {
  const int VEC = dtype ? 8 : 4, Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
  const size_t total = (size_t)B * H * W * (C / VEC);
  DT(hipLaunchKernelGGL(stem_bwd_apply_kernel<float>, dim3(ew_grid(total)), dim3(256), 0, st, (const float*)dpool, idx, (const float*)y, coef, bc, (float*)dy, B, H, W, C, Ho, Wo),
     hipLaunchKernelGGL(stem_bwd_apply_kernel<bf16_t>, dim3(ew_grid(total)), dim3(256), 0, st, (const bf16_t*)dpool, idx, (const bf16_t*)y, coef, bc, (bf16_t*)dy, B, H, W, C, Ho, Wo));
  VQA_LAUNCH_CHECK(); return VQA_OK;
}

int vqa_se_fwd(int dtype, const void* x, const float* w1, const float* w2, float* pooled, float* hidden, float* scale, void* out,
               int B, int HW, int C, int Cr, const float* pool_part, int pool_chunks, hipStream_t st) {
  const int VEC = dtype ? 8 : 4;
  if (!bn_vec_ok(dtype, C) || Cr < 1 || Cr > C) return VQA_EARG;
  if (pool_part && pool_chunks != vqa_bn_apply_pool_chunks(dtype, HW, C)) return VQA_EARG;
  const size_t shm = ((size_t)256 * VEC + C + Cr) * 4;
  DT(hipLaunchKernelGGL(se_pool_fc_kernel<float>, dim3(B), dim3(256), shm, st, (const float*)x, w1, w2, pooled, hidden, scale, HW, C, Cr, pool_part, pool_chunks),
     hipLaunchKernelGGL(se_pool_fc_kernel<bf16_t>, dim3(B), dim3(256), shm, st, (const bf16_t*)x, w1, w2, pooled, hidden, scale, HW, C, Cr, pool_part, pool_chunks));
  const size_t npix = (size_t)B * HW;
  if (npix >= (1ull << 28)) return VQA_EARG;
  DT(hipLaunchKernelGGL(scale_kernel<float>, dim3(px_grid(npix, C, VEC)), dim3(256), 0, st, (const float*)x, scale, (const float*)nullptr, (float*)out, (unsigned)npix, C, magic40(HW)),
     hipLaunchKernelGGL(scale_kernel<bf16_t>, dim3(px_grid(npix, C, VEC)), dim3(256), 0, st, (const bf16_t*)x, scale, (const float*)nullptr, (bf16_t*)out, (unsigned)npix, C, magic40(HW)));
  VQA_LAUNCH_CHECK(); return VQA_OK;
}
// rows of the BatchNorm-backward slab vqa_se_bwd fills when bn_slab is given (= workgroups of its apply pass)
int vqa_se_bwd_blocks(int dtype, int B, int HW, int C) {
  const int VEC = dtype ? 8 : 4;
  if (!bn_vec_ok(dtype, C)) return 0;
  const int g = px_grid((size_t)B * HW, C, VEC);
  return g > 2048 ? 2048 : g;          // slab rows vqa_bn_bwd_finalize folds (it is sized for <= ~1k rows: 16384 rows cost it +90 us)
}
// measurement switch (ablation builds only): VQA_SE_NREG=0 -> the re-reading form of the per-sample SE backward
static bool se_bwd_nreg_off() { return vqa_env_int("VQA_SE_NREG", 1) == 0; }
static bool se_bwd_nlds_off() { return vqa_env_int("VQA_SE_NLDS", 1) == 0; }
// scratch floats vqa_se_bwd needs: dz2[B*C] | dh[B*Cr] | dpool[B*C]
long long vqa_se_bwd_scratch(int dtype, int B, int HW, int C, int Cr) { (void)dtype; (void)HW; return (long long)B * (2 * C + Cr); }
// scratch: vqa_se_bwd_scratch floats
// bn_y / bn_coef / bn_slab (all or none): dx is the gradient entering the BatchNorm whose conv output is bn_y (the last block's bn2,
// mask_out = 1): its backward column sums go to bn_slab[vqa_se_bwd_blocks][3][C] and vqa_bn_bwd_reduce is skipped by the caller.
// bn_acc_mode: 1: bn_slab is a fixed-point accumulator (vqa_bn_acc_words(3, C))
int vqa_se_bwd(int dtype, const void* dout, const void* x, const float* w1, const float* w2, const float* pooled, const float* hidden,
               const float* scale, float* scratch, void* dx, float* dw1, float* dw2, int B, int HW, int C, int Cr, int mask_out,
               const void* bn_y, const float* bn_coef, float* bn_slab, int bn_acc_mode, hipStream_t st) {
  const int VEC = dtype ? 8 : 4;
  // Cr <= C (the model's bottleneck is C / se_reduction) bounds the dynamic LDS of the launches below that do not raise the limit:
  // shm <= shm2 <= (1024 * 8 + 4 * 2048) * 4 = 64 KB at bf16 C = 2048
  if (!bn_vec_ok(dtype, C) || Cr < 1 || Cr > C) return VQA_EARG;
  if ((bn_slab != nullptr) != (bn_y != nullptr) || (bn_slab != nullptr) != (bn_coef != nullptr)) return VQA_EARG;
  if ((dw1 != nullptr) != (dw2 != nullptr)) return VQA_EARG;       // both NULL: data gradient only (frozen SE weights)
  float* dz2 = scratch; float* dh = dz2 + (size_t)B * C; float* dpool = dh + (size_t)B * Cr;
  const int cvh = C / VEC;
  const int nt = (1024 % cvh == 0 && (long long)HW * cvh >= (dtype ? 2048 : 4096)) ? 1024 : 256;      // threads per sample (tiny maps: 256 are plenty; bf16 7 x 7 x 512: 1024, so that a thread keeps all its 4 vectors)
  const size_t shm = ((size_t)nt * VEC + C + Cr) * 4;
  const bool accm = (bn_acc_mode & 1) != 0;
  if (bn_slab && accm && B > VQA_ACC_MAX_PARTS) return VQA_EARG;     // one partial per sample (common.h: the fixed-point total must not wrap)
  if (!bn_slab || accm) {                    // one pass structure: reduce + apply per sample in the same workgroup
    const size_t shm2 = ((size_t)nt * VEC + 3 * C + Cr) * 4;
#define SE_FUSED(TT, R) hipLaunchKernelGGL((se_bwd_fused_kernel<TT, R>), dim3(B), dim3(nt), shm2, st, (const TT*)dout, (const TT*)x, w1, w2, hidden, scale, \
    dz2, dh, dpool, (TT*)dx, HW, C, Cr, mask_out, (const TT*)bn_y, bn_coef, (unsigned long long*)bn_slab)
#define SE_FUSED_K(R_, NR, NL) do { if (tailm) SE_FUSED_KT(R_, NR, NL, true); else SE_FUSED_KT(R_, NR, NL, false); } while (0)
#define SE_FUSED_KT(R_, NR, NL, TM) do { \
      const size_t shl = ((shm2 + 15) & ~(size_t)15) + (size_t)(NL) * nt * 17 + ((TM) ? (size_t)ntail * nt : 0); \
      auto kfn = se_bwd_fused_kernel<bf16_t, R_, NR, NL, TM>; \
      (void)vqa_ensure_lds(reinterpret_cast<const void*>(kfn), shl); \
      hipLaunchKernelGGL(kfn, dim3(B), dim3(nt), shl, st, (const bf16_t*)dout, (const bf16_t*)x, w1, w2, hidden, scale, dz2, dh, dpool, (bf16_t*)dx, \
                         HW, C, Cr, mask_out, (const bf16_t*)bn_y, bn_coef, (unsigned long long*)bn_slab); } while (0)
#define SE_FUSED_D(R_) do { if (nreg == 2) SE_FUSED_K(R_, 2, 0); else if (nlds == 0) SE_FUSED_K(R_, 4, 0); else if (nlds == 2) SE_FUSED_K(R_, 4, 2); \
      else if (nlds == 4) SE_FUSED_K(R_, 4, 4); else SE_FUSED_K(R_, 4, 6); } while (0)
    const int nit = (HW + nt / cvh - 1) / (nt / cvh);          // vectors a thread visits per phase
    const int nreg = !dtype || se_bwd_nreg_off() ? 0 : nit <= 2 ? 2 : 4;       // (8 / 12 kept vectors spill at the 128 registers a 1024-thread workgroup leaves a wave)
    // vectors parked in LDS on top (1024-thread form only: 16 KB each next to the 34 KB of scratch; 6 fill a CU's 160 KB)
    int nlds = (nreg == 4 && nt == 1024 && !se_bwd_nlds_off()) ? (nit <= 4 ? 0 : nit <= 6 ? 2 : nit <= 8 ? 4 : 6) : 0;
    while (nlds > 0 && ((shm2 + 15) & ~(size_t)15) + (size_t)nlds * nt * 17 > 160 * 1024) nlds -= 2;    // (bf16 C = 2048 with a wide Cr: 6 would not fit)
    // one byte of [x > 0] per re-read vector and thread in LDS instead of the second read of x, where it fits beside the rest
    const int ntail = nit - nreg - nlds > 0 ? nit - nreg - nlds : 0;
    const bool tailm = nreg == 4 && mask_out && ntail > 0 && !se_bwd_nlds_off() &&
                       ((shm2 + 15) & ~(size_t)15) + (size_t)nlds * nt * 17 + (size_t)ntail * nt <= 156 * 1024;
    if (dtype && nreg) { if (bn_slab) SE_FUSED_D(true); else SE_FUSED_D(false); }
    else if (dtype) { if (bn_slab) SE_FUSED(bf16_t, true); else SE_FUSED(bf16_t, false); }
    else { if (bn_slab) SE_FUSED(float, true); else SE_FUSED(float, false); }
#undef SE_FUSED_K
#undef SE_FUSED_KT
#undef SE_FUSED_D
#undef SE_FUSED
    if (dw1) launch_se_wgrad(dz2, hidden, dh, pooled, dw1, dw2, B, C, Cr, st);
    VQA_LAUNCH_CHECK(); return VQA_OK;
  }
  DT(hipLaunchKernelGGL(se_bwd_reduce_kernel<float>, dim3(B), dim3(nt), shm, st, (const float*)dout, (const float*)x, w1, w2, hidden, scale, dz2, dh, dpool, HW, C, Cr),
     hipLaunchKernelGGL(se_bwd_reduce_kernel<bf16_t>, dim3(B), dim3(nt), shm, st, (const bf16_t*)dout, (const bf16_t*)x, w1, w2, hidden, scale, dz2, dh, dpool, HW, C, Cr));
  const size_t npix = (size_t)B * HW;
  if (npix >= (1ull << 28)) return VQA_EARG;
  const int ag = bn_slab ? vqa_se_bwd_blocks(dtype, B, HW, C) : px_grid(npix, C, VEC);
#define SE_APPLY(TT, R) hipLaunchKernelGGL((se_bwd_apply_kernel<TT, R>), dim3(ag), dim3(256), 0, st, (const TT*)dout, scale, dpool, (TT*)dx, (unsigned)npix, HW, C, \
    magic40(HW), mask_out ? (const TT*)x : nullptr, (const TT*)bn_y, bn_coef, accm ? nullptr : bn_slab, \
    accm ? (unsigned long long*)bn_slab : nullptr)
  if (dtype) { if (bn_slab) SE_APPLY(bf16_t, true); else SE_APPLY(bf16_t, false); }
  else { if (bn_slab) SE_APPLY(float, true); else SE_APPLY(float, false); }
#undef SE_APPLY
  if (dw1) launch_se_wgrad(dz2, hidden, dh, pooled, dw1, dw2, B, C, Cr, st);
  VQA_LAUNCH_CHECK(); return VQA_OK;
}

int vqa_spatial_fwd(int dtype, const void* x, const float* w, float* pooled2, int* amax, float* amap, void* out, int B, int H, int W, int C, hipStream_t st) {
  const int VEC = dtype ? 8 : 4;
  const size_t npix = (size_t)B * H * W;
  if (!bn_vec_ok(dtype, C) || npix >= (1ull << 28)) return VQA_EARG;      // before any launch: a refused call writes nothing
  const int pg = (int)((npix + 3) / 4 > 8192 ? 8192 : (npix + 3) / 4);
  DT(hipLaunchKernelGGL(spatial_pool_kernel<float>, dim3(pg), dim3(256), 0, st, (const float*)x, pooled2, amax, npix, C),
     hipLaunchKernelGGL(spatial_pool_kernel<bf16_t>, dim3(pg), dim3(256), 0, st, (const bf16_t*)x, pooled2, amax, npix, C));
  hipLaunchKernelGGL(spatial_conv_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, pooled2, w, amap, B, H, W);
  DT(hipLaunchKernelGGL(scale_kernel<float>, dim3(px_grid(npix, C, VEC)), dim3(256), 0, st, (const float*)x, (const float*)nullptr, amap, (float*)out, (unsigned)npix, C, magic40(H * W)),
     hipLaunchKernelGGL(scale_kernel<bf16_t>, dim3(px_grid(npix, C, VEC)), dim3(256), 0, st, (const bf16_t*)x, (const float*)nullptr, amap, (bf16_t*)out, (unsigned)npix, C, magic40(H * W)));
  VQA_LAUNCH_CHECK(); return VQA_OK;
}
// scratch: dpre[B*H*W] | dpool2[B*H*W*2] floats
// floats of the `scratch` argument of vqa_spatial_bwd: dpre [npix] + dpool2 [npix][2] + the conv-weight partial sums [16][98]
long long vqa_spatial_bwd_scratch(int B, int H, int W) { return 3ll * B * H * W + SPATIAL_WG_SLICES * 98; }
int vqa_spatial_bwd(int dtype, const void* dout, const void* x, const float* w, const float* pooled2, const int* amax, const float* amap,
                    float* scratch, void* dx, float* dw, int B, int H, int W, int C, hipStream_t st) {
  const int VEC = dtype ? 8 : 4;
  const size_t npix = (size_t)B * H * W;
  if (!bn_vec_ok(dtype, C) || npix >= (1ull << 28)) return VQA_EARG;      // before any launch: a refused call writes nothing
  float* dpre = scratch; float* dpool2 = dpre + npix; float* wpart = dpool2 + 2 * npix;
  const int pg = (int)((npix + 3) / 4 > 8192 ? 8192 : (npix + 3) / 4);
  DT(hipLaunchKernelGGL(spatial_bwd_reduce_kernel<float>, dim3(pg), dim3(256), 0, st, (const float*)dout, (const float*)x, amap, dpre, npix, C),
     hipLaunchKernelGGL(spatial_bwd_reduce_kernel<bf16_t>, dim3(pg), dim3(256), 0, st, (const bf16_t*)dout, (const bf16_t*)x, amap, dpre, npix, C));
  hipLaunchKernelGGL(spatial_bwd_conv_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, dpre, w, dpool2, B, H, W);
  DT(hipLaunchKernelGGL(spatial_bwd_apply_kernel<float>, dim3(px_grid(npix, C, VEC)), dim3(256), 0, st, (const float*)dout, amap, dpool2, amax, (float*)dx, (unsigned)npix, C),
     hipLaunchKernelGGL(spatial_bwd_apply_kernel<bf16_t>, dim3(px_grid(npix, C, VEC)), dim3(256), 0, st, (const bf16_t*)dout, amap, dpool2, amax, (bf16_t*)dx, (unsigned)npix, C));
  if (dw) {                                  // NULL: data gradient only (frozen conv weight)
    hipLaunchKernelGGL(spatial_wgrad_kernel, dim3(98, SPATIAL_WG_SLICES), dim3(256), 0, st, dpre, pooled2, wpart, B, H, W);
    hipLaunchKernelGGL(spatial_wgrad_finish_kernel, dim3(1), dim3(128), 0, st, wpart, dw);
  }
  VQA_LAUNCH_CHECK(); return VQA_OK;
}

int vqa_nhwc_to_nchw(int dtype, const void* in, float* out, int B, int HW, int C, hipStream_t st) {
  const size_t n = (size_t)B * HW * C;
  DT(hipLaunchKernelGGL(nhwc_to_nchw_kernel<float>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float*)in, out, B, HW, C),
     hipLaunchKernelGGL(nhwc_to_nchw_kernel<bf16_t>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const bf16_t*)in, out, B, HW, C));
  VQA_LAUNCH_CHECK(); return VQA_OK;
}
int vqa_nchw_to_nhwc(int dtype, const float* in, void* out, int B, int HW, int C, hipStream_t st) {
  const size_t n = (size_t)B * HW * C;
  DT(hipLaunchKernelGGL(nchw_to_nhwc_kernel<float>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, in, (float*)out, B, HW, C),
     hipLaunchKernelGGL(nchw_to_nhwc_kernel<bf16_t>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, in, (bf16_t*)out, B, HW, C));
  VQA_LAUNCH_CHECK(); return VQA_OK;
}

}  // extern "C"
