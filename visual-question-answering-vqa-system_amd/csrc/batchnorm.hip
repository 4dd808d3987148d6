// BatchNorm of the residual blocks for gfx950: train statistics, the forward map, the backward.  Split off cnn_ops.hip.  Activations are
// NHWC with T = float | bf16, every per-channel statistic / coefficient is fp32, every global access is a 16-byte vector.
//   BatchNorm2d        models/cnn_backbone.py:151,158,246 (nn.BatchNorm2d defaults)
//   residual add+ReLU  models/cnn_backbone.py:194-195
// One kernel text per form: bn_fwd_kernel<T, RES, POOL, ACC> behind vqa_bn_apply / _pool / _acc, bn_bwd_apply_kernel<T, SELF, DUAL, ACC>
// behind vqa_bn_bwd_apply / _acc, and one masked gradient (bn_bwd_g) in the backward reduce and apply.  The output bits are pinned by
// tests/test_gpu_batchnorm_bits.py, registers and speed against the former three + two kernels by profiles/batchnorm_ab.txt.
// (The stem's BN+ReLU+MaxPool tail, the SE backward's BNRED sums and the conv epilogues that produce the sums live with their kernels.)
#include <type_traits>
#include "common.h"

// ---------------------------------------------------------------------------------------------
// BatchNorm statistics: reduce the igemm partial slab [tiles][2][C] -> mean / invstd / scale / shift
// ---------------------------------------------------------------------------------------------
__global__ void bn_reduce_partials_kernel(const float* __restrict__ part, double* __restrict__ acc, int tiles, int C) {
  // grid (ceil(C/64), G); block 256 = 4 tile-lanes x 64 channels
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), tl = threadIdx.x >> 6;
  __shared__ double sh[2][4][64];
  double s = 0.0, q = 0.0;
  if (c < C) {
    // 8 slab rows in flight per thread: the loop is latency-bound, not bandwidth-bound
    const int step = gridDim.y * 4;
    int t = blockIdx.y * 4 + tl;
    for (; t + 7 * step < tiles; t += 8 * step) {
      float a[8], b[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) { a[u] = part[((size_t)(t + u * step) * 2) * C + c]; b[u] = part[((size_t)(t + u * step) * 2 + 1) * C + c]; }
#pragma unroll
      for (int u = 0; u < 8; ++u) { s += (double)a[u]; q += (double)b[u]; }
    }
    for (; t < tiles; t += step) {
      s += (double)part[((size_t)t * 2) * C + c];
      q += (double)part[((size_t)t * 2 + 1) * C + c];
    }
  }
  sh[0][tl][threadIdx.x & 63] = s; sh[1][tl][threadIdx.x & 63] = q;
  __syncthreads();
  if (tl == 0 && c < C) {
    for (int i = 1; i < 4; ++i) { s += sh[0][i][threadIdx.x]; q += sh[1][i][threadIdx.x]; }
    acc[((size_t)blockIdx.y * 2) * C + c] = s;
    acc[((size_t)blockIdx.y * 2 + 1) * C + c] = q;
  }
}

// coef layout (fp32, 4*C): scale | shift | mean | invstd
__global__ void bn_finalize_kernel(const double* __restrict__ acc, int G, int C, double count, const float* __restrict__ gamma,
                                   const float* __restrict__ beta, float* running_mean, float* running_var, long long* nbt,
                                   float momentum, float eps, float* __restrict__ coef) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double s = 0.0, q = 0.0;
  int g = 0;
  for (; g + 8 <= G; g += 8) {
    double a[8], b[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) { a[u] = acc[((size_t)(g + u) * 2) * C + c]; b[u] = acc[((size_t)(g + u) * 2 + 1) * C + c]; }
#pragma unroll
    for (int u = 0; u < 8; ++u) { s += a[u]; q += b[u]; }
  }
  for (; g < G; ++g) { s += acc[((size_t)g * 2) * C + c]; q += acc[((size_t)g * 2 + 1) * C + c]; }
  const double mean = s / count;
  double var = q / count - mean * mean;
  if (var < 0.0) var = 0.0;
  const float invstd = (float)(1.0 / sqrt(var + (double)eps));
  const float sc = gamma[c] * invstd;
  coef[c] = sc; coef[C + c] = beta[c] - (float)mean * sc; coef[2 * C + c] = (float)mean; coef[3 * C + c] = invstd;
  if (running_mean) {
    const double unbiased = count > 1.0 ? var * count / (count - 1.0) : var;
    running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * (float)mean;
    running_var[c] = (1.f - momentum) * running_var[c] + momentum * (float)unbiased;
    if (c == 0 && nbt) *nbt += 1;
  }
}

__global__ void bn_eval_coef_kernel(int C, const float* gamma, const float* beta, const float* rm, const float* rv, float eps, float* coef) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float invstd = 1.0f / sqrtf(rv[c] + eps);
  const float sc = gamma[c] * invstd;
  coef[c] = sc; coef[C + c] = beta[c] - rm[c] * sc; coef[2 * C + c] = rm[c]; coef[3 * C + c] = invstd;
}

// ---------------------------------------------------------------------------------------------
// Forward: out = [relu]( y*scale+shift  [+ res*rscale+rshift | + res] ).  Each thread owns one 16-byte channel vector (coefficients
// stay in registers) and walks rows; a block covers 256/cv consecutive rows = one contiguous span.
//   RES   0 = none, 1 = + res (identity), 2 = + res*rscale+rshift (the 1x1 shortcut's BatchNorm)
//   POOL  the LAST residual block of a stage, with the squeeze-excitation global average pool folded in (models/cnn_backbone.py:194-197
//         -> models/attention_modules.py:109-112): grid (chunks, B), a workgroup owns rows [chunk*rpc, (chunk+1)*rpc) of ONE sample and
//         also writes the column sums of the values it stores (bf16-rounded, exactly what a pooling pass would read back) to
//         part[b][chunk][C]; se_pool_fc_kernel folds the chunks in index order.  Saves the pooling pass's read of the stage output.
//   ACC   train mode, the batch statistics arrive as fixed-point accumulators (common.h acc_add_fixed; filled by the conv kernel's
//         epilogue): every workgroup finalizes the coefficients of all channels in the prologue (fp64, same formulas as
//         bn_finalize_kernel; BnAcc / bn_acc_coef: common.h -- shared with the stage-1 patch kernels), the first workgroup also
//         publishes coef[4][C] (scale | shift | mean | invstd: the backward reads it) and updates running_mean / running_var /
//         num_batches_tracked (nn.BatchNorm2d defaults).  No finalize launch in between.  Otherwise f / fr are coef[4][C] arrays.
// The coefficient source is the only difference between the forms.  The row index is an int in the pool form without accumulators
// and a size_t elsewhere: with one type for all, bf16 RES 2 of that form takes 90 registers against 76 (profiles/batchnorm_ab.txt B).
// ---------------------------------------------------------------------------------------------
template <bool ACC> using BnSrc = std::conditional_t<ACC, BnAcc, const float*>;
// What a form reads beyond the five pointers: the kernel's trailing arguments A..., one by one and in this order, so that a form's
// argument block holds nothing it does not read (a plain form that carried the others' arguments loaded rows | C | relu in two pieces
// and was 0.2 .. 2 us slower per launch; as a device function behind three kernels the text lost a register in ACC RES 2: record, B)
template <bool POOL, bool ACC> struct BnFwdArgs { size_t rows; int HW, C, relu, rpc; double inv_count, unbias; float momentum, eps; float* part; };
template <> struct BnFwdArgs<false, false> { size_t rows; int C, relu; };
template <> struct BnFwdArgs<true, false> { int HW, C, relu, rpc; float* part; };

template <typename T, int RES, bool POOL, bool ACC, typename... A>
__global__ __launch_bounds__(256) void bn_fwd_kernel(const T* __restrict__ y, BnSrc<ACC> f, const T* __restrict__ res, BnSrc<ACC> fr,
                                                     T* __restrict__ out, A... args) {
  static_assert(!(POOL && ACC && RES == 2), "vqa_bn_apply_acc refuses pool_part together with racc");
  static_assert(sizeof...(A) == (ACC ? 10 : POOL ? 5 : 3), "one argument per member of BnFwdArgs<POOL, ACC>");
  const BnFwdArgs<POOL, ACC> a = {args...};
  const int C = a.C, relu = a.relu;
  constexpr int VEC = Vec16<T>::N;
  const int cv = C / VEC, lanes_r = 256 / cv;
  const int c0 = (threadIdx.x % cv) * VEC, myr = threadIdx.x / cv;
  float sc[VEC], sh[VEC], rs[RES == 2 ? VEC : 1], rh[RES == 2 ? VEC : 1], acc[POOL ? VEC : 1];
  if constexpr (ACC) {
    const bool writer = blockIdx.x == 0 && blockIdx.y == 0;
    extern __shared__ float cf[];                // [2 | 4][C]: scale, shift (, residual scale, shift)
    for (int c = threadIdx.x; c < C; c += 256) {
      bn_acc_coef(f, C, c, a.inv_count, a.unbias, a.momentum, a.eps, writer, cf[c], cf[C + c]);
      if (RES == 2) bn_acc_coef(fr, C, c, a.inv_count, a.unbias, a.momentum, a.eps, writer, cf[2 * C + c], cf[3 * C + c]);
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      sc[j] = cf[c0 + j]; sh[j] = cf[C + c0 + j];
      if (RES == 2) { rs[j] = cf[2 * C + c0 + j]; rh[j] = cf[3 * C + c0 + j]; }
    }
  } else {
    const float* __restrict__ coef = f; const float* __restrict__ rcoef = fr;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      sc[j] = coef[c0 + j]; sh[j] = coef[C + c0 + j];
      if (RES == 2) { rs[j] = rcoef[c0 + j]; rh[j] = rcoef[C + c0 + j]; }
    }
  }
  if (POOL) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[j] = 0.f;
  }
  std::conditional_t<POOL && !ACC, int, size_t> r, r1, rstep;
  size_t base = c0;
  if constexpr (POOL) { const int r0 = blockIdx.x * a.rpc; r = r0 + myr; r1 = min(a.HW, r0 + a.rpc); rstep = lanes_r; base += (size_t)blockIdx.y * a.HW * C; }
  else { r = (size_t)blockIdx.x * lanes_r + myr; r1 = a.rows; rstep = (size_t)gridDim.x * lanes_r; }
#pragma unroll 2
  for (; r < r1; r += rstep) {
    const size_t off = base + (size_t)r * C;
    Vec16<T> v = ldg16(y + off), rr, o;
    if (RES) rr = ldg16(res + off);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      float x = v.get(j) * sc[j] + sh[j];
      if (RES == 1) x += rr.get(j);
      if (RES == 2) x += rr.get(j) * rs[j] + rh[j];
      o.set(j, (relu && x < 0.f) ? 0.f : x);   // NaN-propagating ReLU like torch
      if (POOL) acc[j] += o.get(j);
    }
    stg16(out + off, o);
  }
  if constexpr (POOL) {
    __shared__ float shs[256 * VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) shs[threadIdx.x * VEC + j] = acc[j];
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
      const int v = c / VEC, j = c - v * VEC;
      float t = 0.f;
      for (int q = 0; q < lanes_r; ++q) t += shs[(q * cv + v) * VEC + j];
      a.part[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * C + c] = t;
    }
  }
}
// ---------------------------------------------------------------------------------------------
// BatchNorm backward.  g = dout * (out > 0) (relu) or dout.  Partial sums per block -> slab [blocks][3][C]:
//   0: sum g   1: sum g*xhat(y)   2: sum g*xhat(y2) (second BN sharing g: the 1x1 shortcut)
// ---------------------------------------------------------------------------------------------
// The masked gradient of element j.  SELF: the ReLU mask is relu(bn(y)) > 0 recomputed from y with ms | mh (scale, shift);
// otherwise outact > 0 (o: its vector) where the launch has an outact, or none.
template <typename T, bool SELF>
__device__ __forceinline__ float bn_bwd_g(const Vec16<T>& d, const Vec16<T>& yy, const T* outact, const Vec16<T>& o, const float* ms, const float* mh, int j) {
  float g = d.get(j);
  if constexpr (SELF) { if (!(yy.get(j) * ms[j] + mh[j] > 0.f)) g = 0.f; }
  else if (outact && !(o.get(j) > 0.f)) g = 0.f;
  return g;
}

template <typename T, bool SELF, bool DUAL>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const T* __restrict__ dout, const T* __restrict__ outact, const T* __restrict__ y,
                                                            const float* __restrict__ coef, const T* __restrict__ y2,
                                                            const float* __restrict__ coef2, float* __restrict__ slab, size_t rows, int C,
                                                            unsigned long long* __restrict__ facc) {
  constexpr int VEC = Vec16<T>::N;
  const int cv = C / VEC;                 // vectors per row
  const int lanes_r = 256 / cv;           // rows processed concurrently by the block (C <= 256*VEC)
  const int myv = threadIdx.x % cv, myr = threadIdx.x / cv, c0 = myv * VEC;
  float sg[VEC], sx[VEC], sx2[DUAL ? VEC : 1], mean[VEC], inv[VEC], ms[SELF ? VEC : 1], mh[SELF ? VEC : 1], mean2[DUAL ? VEC : 1], inv2[DUAL ? VEC : 1];
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    sg[j] = sx[j] = 0.f; mean[j] = coef[2 * C + c0 + j]; inv[j] = coef[3 * C + c0 + j];
    if (DUAL) { sx2[j] = 0.f; mean2[j] = coef2[2 * C + c0 + j]; inv2[j] = coef2[3 * C + c0 + j]; }
    if (SELF) { ms[j] = coef[c0 + j]; mh[j] = coef[C + c0 + j]; }
  }
#pragma unroll 2
  for (size_t r = (size_t)blockIdx.x * lanes_r + myr; r < rows; r += (size_t)gridDim.x * lanes_r) {
    const size_t off = r * C + c0;
    Vec16<T> d = ldg16(dout + off), yy = ldg16(y + off), o, y2v;
    if (!SELF && outact) o = ldg16(outact + off);
    if (DUAL) y2v = ldg16(y2 + off);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const float g = bn_bwd_g<T, SELF>(d, yy, outact, o, ms, mh, j);
      sg[j] += g;
      sx[j] += g * (yy.get(j) - mean[j]) * inv[j];
      if (DUAL) sx2[j] += g * (y2v.get(j) - mean2[j]) * inv2[j];
    }
  }
  extern __shared__ float shm[];          // [3][256][VEC]
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    shm[(0 * 256 + threadIdx.x) * VEC + j] = sg[j];
    shm[(1 * 256 + threadIdx.x) * VEC + j] = sx[j];
    shm[(2 * 256 + threadIdx.x) * VEC + j] = DUAL ? sx2[j] : 0.f;
  }
  __syncthreads();
  for (int o = threadIdx.x; o < 3 * C; o += 256) {
    const int k = o / C, c = o - k * C, v = c / VEC, j = c - v * VEC;
    float s = 0.f;
    for (int r = 0; r < lanes_r; ++r) s += shm[(k * 256 + r * cv + v) * VEC + j];
    if (facc) {                               // fixed point: order-free, no finalize launch; replica blockIdx.x % R
      const int R = acc_replicas(C);
      if (k < 2 || DUAL) acc_add_fixed(facc, (size_t)R * 3 * C, ((size_t)(blockIdx.x % R) * 3 + k) * C + c, s);
    }
    else slab[((size_t)blockIdx.x * 3 + k) * C + c] = s;
  }
}

// The apply coefficients of one channel in training mode, dy = A*g + B*y + C, from gi = gamma * invstd and the column means
// mg = sum g / count, mgx = sum g*xhat / count.  (How the means are formed stays with each caller: bn_bwd_finalize_kernel divides
// by count in fp64, the accumulator prologue multiplies by 1 / count; they round differently.)
__device__ __forceinline__ void bn_bwd_abc(float gi, float mean, float invstd, float mg, float mgx, float& a, float& b, float& c) {
  a = gi; b = -gi * invstd * mgx; c = gi * (mean * invstd * mgx - mg);
}

// reduce slab over blocks; emit dgamma/dbeta (+=) and the apply coefficients  dy = A*g + Bc*y + Cc
// bcoef layout (3*C): A | Bc | Cc
__global__ __launch_bounds__(1024) void bn_bwd_finalize_kernel(const float* __restrict__ slab, int nblk, int C, int which, double count,
                                       const float* __restrict__ gamma, const float* __restrict__ coef, int training,
                                       float* dgamma, float* dbeta, float* __restrict__ bcoef) {
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), tl = threadIdx.x >> 6;
  __shared__ double sh[2][16][64];
  double sg = 0.0, sx = 0.0;
  if (c < C) {
    int b = tl;
    for (; b + 7 * 16 < nblk; b += 8 * 16) {               // 8 slab rows in flight per thread (latency-bound loop)
      float a[8], x[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) { a[u] = slab[((size_t)(b + 16 * u) * 3) * C + c]; x[u] = slab[((size_t)(b + 16 * u) * 3 + which) * C + c]; }
#pragma unroll
      for (int u = 0; u < 8; ++u) { sg += a[u]; sx += x[u]; }
    }
    for (; b < nblk; b += 16) { sg += slab[((size_t)b * 3) * C + c]; sx += slab[((size_t)b * 3 + which) * C + c]; }
  }
  sh[0][tl][threadIdx.x & 63] = sg; sh[1][tl][threadIdx.x & 63] = sx;
  __syncthreads();
  if (tl != 0 || c >= C) return;
  for (int i = 1; i < 16; ++i) { sg += sh[0][i][threadIdx.x]; sx += sh[1][i][threadIdx.x]; }
  if (dgamma) dgamma[c] += (float)sx;
  if (dbeta) dbeta[c] += (float)sg;
  const float mean = coef[2 * C + c], invstd = coef[3 * C + c], gi = gamma[c] * invstd;
  if (training) bn_bwd_abc(gi, mean, invstd, (float)(sg / count), (float)(sx / count), bcoef[c], bcoef[C + c], bcoef[2 * C + c]);
  else { bcoef[c] = gi; bcoef[C + c] = 0.f; bcoef[2 * C + c] = 0.f; }
}

// dy = A*g + B*y + C ; optional second output dy2 = A2*g + B2*y2 + C2 (DUAL: the 1x1 shortcut's BatchNorm sharing g).
// SELF: the ReLU mask is recomputed from y with scale | shift; otherwise outact > 0 (or none): bn_bwd_g.  Specialised so unused
// coefficient sets cost no registers.
//   ACC = false   s1 / s2 are bc / bc2 (A | B | C, vqa_bn_bwd_finalize) and mask_or_count is mcoef (scale | shift) for SELF.
//   ACC = true    the finalize folded into the prologue: the column sums arrive as a fixed-point accumulator facc[vqa_bn_acc_words(3, C)]
//                 (R replicas x [3][C] in a hi and a lo plane, the flag word between the planes: common.h); every workgroup derives
//                 A | B | C of all channels once (bn_bwd_abc, training mode) and shares them through LDS, the first workgroup adds
//                 d gamma / d beta (and the shortcut BatchNorm's, DUAL) into the gradient buffer.  mask_or_count is 1 / count.
// The arguments stand in the order both former kernels had them.
struct BnBwdSide { const float* gamma; const float* coef; float* dgamma; float* dbeta; };
struct BnBwdAcc { const unsigned long long* facc; BnBwdSide s; };
template <bool ACC> using BnBwdSrc1 = std::conditional_t<ACC, BnBwdAcc, const float*>;
template <bool ACC> using BnBwdSrc2 = std::conditional_t<ACC, BnBwdSide, const float*>;

template <typename T, bool SELF, bool DUAL, bool ACC>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const T* __restrict__ dout, const T* __restrict__ outact, const T* __restrict__ y,
                                    BnBwdSrc1<ACC> s1, T* __restrict__ dy, const T* __restrict__ y2, BnBwdSrc2<ACC> s2, T* __restrict__ dy2,
                                    size_t rows, int C, std::conditional_t<ACC, double, const float*> mask_or_count) {
  constexpr int VEC = Vec16<T>::N;
  const int cv = C / VEC, lanes_r = 256 / cv;
  const int c0 = (threadIdx.x % cv) * VEC, myr = threadIdx.x / cv;
  float a[VEC], b[VEC], c[VEC], a2[DUAL ? VEC : 1], b2[DUAL ? VEC : 1], c2[DUAL ? VEC : 1], ms[SELF ? VEC : 1], mh[SELF ? VEC : 1];
  if constexpr (ACC) {
    const unsigned long long* __restrict__ facc = s1.facc;
    const double inv_count = mask_or_count;
    const bool writer = blockIdx.x == 0;
    const int R = acc_replicas(C);
    const bool bad = acc_flagged(facc, R, 3, C);
    extern __shared__ float cf[];                // [3 | 6][C]: A, B, C (, A2, B2, C2): one evaluation per channel and workgroup
    for (int ch = threadIdx.x; ch < C; ch += 256) {
      double sg = acc_read_fixed(facc, R, 3, C, 0, ch), sx = acc_read_fixed(facc, R, 3, C, 1, ch);
      if (bad) sg = sx = __builtin_nan("");
      const float mean = s1.s.coef[2 * C + ch], invstd = s1.s.coef[3 * C + ch], gi = s1.s.gamma[ch] * invstd;
      const float mg = (float)(sg * inv_count);
      bn_bwd_abc(gi, mean, invstd, mg, (float)(sx * inv_count), cf[ch], cf[C + ch], cf[2 * C + ch]);
      if (writer) { s1.s.dgamma[ch] += (float)sx; s1.s.dbeta[ch] += (float)sg; }
      if (DUAL) {
        double sx2 = acc_read_fixed(facc, R, 3, C, 2, ch);
        if (bad) sx2 = __builtin_nan("");
        const float mean2 = s2.coef[2 * C + ch], inv2 = s2.coef[3 * C + ch], gi2 = s2.gamma[ch] * inv2;
        bn_bwd_abc(gi2, mean2, inv2, mg, (float)(sx2 * inv_count), cf[3 * C + ch], cf[4 * C + ch], cf[5 * C + ch]);
        if (writer) { s2.dgamma[ch] += (float)sx2; s2.dbeta[ch] += (float)sg; }
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const int ch = c0 + j;
      a[j] = cf[ch]; b[j] = cf[C + ch]; c[j] = cf[2 * C + ch];
      if (DUAL) { a2[j] = cf[3 * C + ch]; b2[j] = cf[4 * C + ch]; c2[j] = cf[5 * C + ch]; }
      if (SELF) { ms[j] = s1.s.coef[ch]; mh[j] = s1.s.coef[C + ch]; }
    }
  } else {
    const float* __restrict__ bc = s1; const float* __restrict__ bc2 = s2; const float* __restrict__ mcoef = mask_or_count;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      a[j] = bc[c0 + j]; b[j] = bc[C + c0 + j]; c[j] = bc[2 * C + c0 + j];
      if (DUAL) { a2[j] = bc2[c0 + j]; b2[j] = bc2[C + c0 + j]; c2[j] = bc2[2 * C + c0 + j]; }
      if (SELF) { ms[j] = mcoef[c0 + j]; mh[j] = mcoef[C + c0 + j]; }
    }
  }
#pragma unroll 2
  for (size_t r = (size_t)blockIdx.x * lanes_r + myr; r < rows; r += (size_t)gridDim.x * lanes_r) {
    const size_t off = r * C + c0;
    Vec16<T> d = ldg16(dout + off), yy = ldg16(y + off), o, y2v, rr, r2;
    if (!SELF && outact) o = ldg16(outact + off);
    if (DUAL) y2v = ldg16(y2 + off);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const float g = bn_bwd_g<T, SELF>(d, yy, outact, o, ms, mh, j);
      rr.set(j, a[j] * g + b[j] * yy.get(j) + c[j]);
      if (DUAL) r2.set(j, a2[j] * g + b2[j] * y2v.get(j) + c2[j]);
    }
    stg16(dy + off, rr);
    if (DUAL) stg16(dy2 + off, r2);
  }
}

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
static inline int row_grid(size_t rows, int lanes_r) { size_t g = (rows + lanes_r - 1) / lanes_r; return (int)(g > 8192 ? 8192 : (g ? g : 1)); }
// rows of one sample a workgroup of the pooling forward owns (14 passes of the workgroup)
static inline int pool_rpc(int C, int VEC) { return (256 / (C / VEC)) * 14; }

// (dtype, mode) -> fn(BnType<float | bf16_t>, std::integral_constant<int, mode>) for the listed modes: a launch site names its
// instantiation from the two tags (BN_T, BN_M).  A mode outside the list launches nothing (the entries compute the mode themselves).
template <typename T> struct BnType { using type = T; };
template <int M0, int... Ms, typename F>
static inline void bn_dispatch(int dtype, int mode, F&& fn) {
  if (mode == M0) { if (dtype) fn(BnType<bf16_t>{}, std::integral_constant<int, M0>{}); else fn(BnType<float>{}, std::integral_constant<int, M0>{}); }
  else if constexpr (sizeof...(Ms) > 0) bn_dispatch<Ms...>(dtype, mode, fn);
}
#define BN_T typename decltype(t)::type
#define BN_M decltype(m)::value
// backward: 0 plain | 1 SELF | 2 DUAL
static inline int bn_mask_mode(bool self_mask, const void* y2) { return self_mask ? 1 : (y2 ? 2 : 0); }
// forward: 0 none | 1 + res | 2 + BatchNorm(res) (rsrc: the residual's own coefficients or accumulators are given)
static inline int bn_res_mode(const void* res, const void* rsrc) { return !res ? 0 : (rsrc ? 2 : 1); }

extern "C" {

// part: igemm slab [tiles][2][C]; scratch: >= 64*2*C doubles; coef out: 4*C floats. running_* / nbt may be null.
int vqa_bn_stats_finalize(const float* part, int tiles, int C, double count, const float* gamma, const float* beta,
                          float* running_mean, float* running_var, long long* nbt, float momentum, float eps,
                          double* scratch, float* coef, hipStream_t st) {
  if (!part || !scratch || !coef || tiles <= 0 || C <= 0) return VQA_EARG;
  int G = (tiles + 63) / 64; if (G > 64) G = 64; if (G < 1) G = 1;
  hipLaunchKernelGGL(bn_reduce_partials_kernel, dim3((C + 63) / 64, G), dim3(256), 0, st, part, scratch, tiles, C);
  hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + 255) / 256), dim3(256), 0, st, scratch, G, C, count, gamma, beta,
                     running_mean, running_var, nbt, momentum, eps, coef);
  VQA_LAUNCH_CHECK(); return VQA_OK;
}
int vqa_bn_eval_coef(int C, const float* gamma, const float* beta, const float* rm, const float* rv, float eps, float* coef, hipStream_t st) {
  hipLaunchKernelGGL(bn_eval_coef_kernel, dim3((C + 255) / 256), dim3(256), 0, st, C, gamma, beta, rm, rv, eps, coef);
  VQA_LAUNCH_CHECK(); return VQA_OK;
}
// out = [relu](y*scale + shift [+ res | + res*rscale + rshift]) with given coefficients coef / rcoef [4][C] (eval mode, or after
// vqa_bn_stats_finalize).  res NULL: no residual; rcoef NULL: the identity residual.
int vqa_bn_apply(int dtype, const void* y, const float* coef, const void* res, const float* rcoef, void* out, long long numel, int C, int relu, hipStream_t st) {
  if (!bn_vec_ok(dtype, C) || numel % C) return VQA_EARG;
  const size_t rows = (size_t)numel / C;
  const int grid = row_grid(rows, 256 / (C / (dtype ? 8 : 4)));
  bn_dispatch<0, 1, 2>(dtype, bn_res_mode(res, rcoef), [&](auto t, auto m) {
    hipLaunchKernelGGL((bn_fwd_kernel<BN_T, BN_M, false, false, size_t, int, int>), dim3(grid), dim3(256), 0, st, (const BN_T*)y, coef, (const BN_T*)res, rcoef, (BN_T*)out, rows, C, relu);
  });
  VQA_LAUNCH_CHECK(); return VQA_OK;
}
// chunks per sample of the pooling forward (0: a shape it refuses)
int vqa_bn_apply_pool_chunks(int dtype, int HW, int C) {
  if (!bn_vec_ok(dtype, C) || HW <= 0) return 0;
  const int rpc = pool_rpc(C, dtype ? 8 : 4);
  return (HW + rpc - 1) / rpc;
}
// bn_apply of a stage's last block + the SE pooling sums: part [B][vqa_bn_apply_pool_chunks][C] floats (vqa_se_fwd folds them)
int vqa_bn_apply_pool(int dtype, const void* y, const float* coef, const void* res, const float* rcoef, void* out, int B, int HW, int C,
                      int relu, float* part, hipStream_t st) {
  const int chunks = vqa_bn_apply_pool_chunks(dtype, HW, C);
  if (!y || !coef || !out || !part || B <= 0 || chunks <= 0 || B > 65535) return VQA_EARG;
  const int rpc = pool_rpc(C, dtype ? 8 : 4);
  bn_dispatch<0, 1, 2>(dtype, bn_res_mode(res, rcoef), [&](auto t, auto m) {
    hipLaunchKernelGGL((bn_fwd_kernel<BN_T, BN_M, true, false, int, int, int, int, float*>), dim3(chunks, B), dim3(256), 0, st, (const BN_T*)y, coef, (const BN_T*)res, rcoef, (BN_T*)out,
                       HW, C, relu, rpc, part);
  });
  VQA_LAUNCH_CHECK(); return VQA_OK;
}
// 64-bit words of a fixed-point accumulator for K sums of C channels (replicas + flag, even): what the caller zeroes and passes
int vqa_bn_acc_words(int K, int C) { const long long w = 2ll * acc_replicas(C) * K * C + 1; return (int)((w + 1) / 2 * 2); }   // hi plane | flag | lo plane (common.h)
// Train-mode BatchNorm apply whose statistics are fixed-point accumulators acc[vqa_bn_acc_words(2, C)] (filled by the producing conv launched
// with stats_mode = 1): finalize + running-statistics update + apply (+ residual | + BatchNorm(res) from racc, + ReLU) in ONE launch;
// coef_out / rcoef_out [4][C] are published for the backward.  pool_part != NULL: the SE-pooling variant (vqa_bn_apply_pool).
int vqa_bn_apply_acc(int dtype, const void* y, const unsigned long long* acc, const float* gamma, const float* beta, float* rm, float* rv,
                     long long* nbt, float* coef_out, const void* res, const unsigned long long* racc, const float* rgamma, const float* rbeta,
                     float* rrm, float* rrv, long long* rnbt, float* rcoef_out, void* out, int B, int HW, int C, int relu, double count,
                     float momentum, float eps, float* pool_part, hipStream_t st) {
  const int VEC = dtype ? 8 : 4;
  if (!y || !acc || !gamma || !beta || !coef_out || !out || B <= 0 || HW <= 0 || !bn_vec_ok(dtype, C)) return VQA_EARG;
  if (racc && (!res || !rgamma || !rbeta || !rcoef_out)) return VQA_EARG;
  if (pool_part && racc) return VQA_EARG;
  BnAcc f = {acc, gamma, beta, rm, rv, nbt, coef_out}, fr = {racc, rgamma, rbeta, rrm, rrv, rnbt, rcoef_out};
  const size_t rows = (size_t)B * HW;
  int g1 = row_grid(rows, 256 / (C / VEC));
  // every workgroup finalizes all C channels in its prologue (R replicas x 2 planes x 2 sums of 8-byte loads + fp64 per channel): with 2048
  // workgroups the prologues read more bytes than the stage-4 tensor holds.  tools/bn_grid_sweep.py, B = 512: 1024 (plain) / 512 (+ residual)
  // workgroups are 3 .. 18 % faster than 2048 at every stage; 256 loses the latency cover again
  { const int cap = vqa_env_int("VQA_BN_GRID", res ? 512 : 1024); if (g1 > cap) g1 = cap; }
  dim3 grid(g1);
  int rpc = 0;
  const size_t shm = (size_t)(racc ? 4 : 2) * C * sizeof(float);
  if (pool_part) {
    const int chunks = vqa_bn_apply_pool_chunks(dtype, HW, C);
    if (chunks <= 0 || B > 65535) return VQA_EARG;
    rpc = pool_rpc(C, VEC); grid = dim3(chunks, B);
  }
  const double inv_count = 1.0 / count, unbias = count > 1.0 ? count / (count - 1.0) : 1.0;
  // mode 3 | 4: RES 0 | 1 with the SE pooling (RES 2 with it was refused above, and has no instantiation)
  bn_dispatch<0, 1, 2, 3, 4>(dtype, bn_res_mode(res, racc) + (pool_part ? 3 : 0), [&](auto t, auto m) {
    hipLaunchKernelGGL((bn_fwd_kernel<BN_T, BN_M % 3, (BN_M >= 3), true, size_t, int, int, int, int, double, double, float, float, float*>), grid, dim3(256), shm, st, (const BN_T*)y, f, (const BN_T*)res, fr, (BN_T*)out,
                       rows, HW, C, relu, rpc, inv_count, unbias, momentum, eps, pool_part);
  });
  VQA_LAUNCH_CHECK(); return VQA_OK;
}
int vqa_bn_bwd_blocks(long long rows) { long long g = (rows + 63) / 64; const int cap = vqa_env_int("VQA_BNR_GRID", rows < 65536 ? 256 : 512); return (int)(g > cap ? cap : (g < 1 ? 1 : g)); }
// slab: [vqa_bn_bwd_blocks(rows)][3][C] floats
// acc_mode = 1: `slab` is a fixed-point accumulator unsigned long long [vqa_bn_acc_words(3, C)] (replicas x two planes + flag, common.h; zeroed by the
// caller) instead of a float slab
int vqa_bn_bwd_reduce(int dtype, const void* dout, const void* outact, const void* y, const float* coef, const void* y2, const float* coef2,
                      float* slab, long long rows, int C, int self_mask, int acc_mode, hipStream_t st) {
  if (!bn_vec_ok(dtype, C)) return VQA_EARG;
  const int nb = vqa_bn_bwd_blocks(rows);
  const size_t shm = (size_t)3 * 256 * (dtype ? 8 : 4) * 4;
  if (self_mask && (y2 || outact)) return VQA_EARG;
  bn_dispatch<0, 1, 2>(dtype, bn_mask_mode(self_mask, y2), [&](auto t, auto m) {
    hipLaunchKernelGGL((bn_bwd_reduce_kernel<BN_T, BN_M == 1, BN_M == 2>), dim3(nb), dim3(256), shm, st, (const BN_T*)dout, (const BN_T*)outact,
                       (const BN_T*)y, coef, (const BN_T*)y2, coef2, acc_mode ? nullptr : slab, (size_t)rows, C, acc_mode ? (unsigned long long*)slab : nullptr);
  });
  VQA_LAUNCH_CHECK(); return VQA_OK;
}
// slab [nblk][3][C] -> bcoef [3][C] of BatchNorm `which` (1: sum g*xhat(y), 2: the shortcut's), dgamma / dbeta += (either may be NULL);
// training = 0: eval-mode / frozen statistics (dy = gamma * invstd * g)
int vqa_bn_bwd_finalize(const float* slab, int nblk, int C, int which, double count, const float* gamma, const float* coef, int training,
                        float* dgamma, float* dbeta, float* bcoef, hipStream_t st) {
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((C + 63) / 64), dim3(1024), 0, st, slab, nblk, C, which, count, gamma, coef, training, dgamma, dbeta, bcoef);
  VQA_LAUNCH_CHECK(); return VQA_OK;
}
// BatchNorm backward apply with the finalize folded in (training mode): facc[vqa_bn_acc_words(3, C)] fixed-point sums from vqa_bn_bwd_reduce /
// vqa_se_bwd in accumulate mode; d gamma / d beta (+=) are written by the first workgroup.  y2 / gamma2 / coef2 / dgamma2 / dbeta2 / dy2:
// the 1x1 shortcut's BatchNorm sharing g (all or none).  self_mask: ReLU mask recomputed from y (coef scale | shift), outact unused.
int vqa_bn_bwd_apply_acc(int dtype, const void* dout, const void* outact, const void* y, const unsigned long long* facc, const float* gamma,
                         const float* coef, float* dgamma, float* dbeta, void* dy, const void* y2, const float* gamma2, const float* coef2,
                         float* dgamma2, float* dbeta2, void* dy2, long long numel, int C, double count, int self_mask, hipStream_t st) {
  if (!dout || !y || !facc || !gamma || !coef || !dgamma || !dbeta || !dy || !bn_vec_ok(dtype, C) || numel % C) return VQA_EARG;
  if (y2 && (!gamma2 || !coef2 || !dgamma2 || !dbeta2 || !dy2)) return VQA_EARG;
  if (self_mask && (y2 || outact)) return VQA_EARG;
  const size_t rows = (size_t)numel / C;
  int grid = row_grid(rows, 256 / (C / (dtype ? 8 : 4)));
  { const int cap = vqa_env_int("VQA_BNB_GRID", 512); if (grid > cap) grid = cap; }     // (prologue amortisation, as vqa_bn_apply_acc: -4 .. -20 % against 2048)
  const size_t shm = (size_t)(y2 ? 6 : 3) * C * sizeof(float);
  const BnBwdAcc s1 = {facc, {gamma, coef, dgamma, dbeta}};
  const BnBwdSide s2 = {gamma2, coef2, dgamma2, dbeta2};
  const double inv_count = 1.0 / count;
  bn_dispatch<0, 1, 2>(dtype, bn_mask_mode(self_mask, y2), [&](auto t, auto m) {
    hipLaunchKernelGGL((bn_bwd_apply_kernel<BN_T, BN_M == 1, BN_M == 2, true>), dim3(grid), dim3(256), shm, st, (const BN_T*)dout, (const BN_T*)outact,
                       (const BN_T*)y, s1, (BN_T*)dy, (const BN_T*)y2, s2, (BN_T*)dy2, rows, C, inv_count);
  });
  VQA_LAUNCH_CHECK(); return VQA_OK;
}
// dy = bc0*g + bc1*y + bc2 with given coefficients bc [3][C] (vqa_bn_bwd_finalize); y2 / bc2 / dy2: the shortcut's BatchNorm sharing g;
// mask_coef (scale | shift): the ReLU mask recomputed from y instead of outact > 0
int vqa_bn_bwd_apply(int dtype, const void* dout, const void* outact, const void* y, const float* bc, void* dy,
                     const void* y2, const float* bc2, void* dy2, long long numel, int C, const float* mask_coef, hipStream_t st) {
  if (!bn_vec_ok(dtype, C) || numel % C) return VQA_EARG;
  const size_t rows = (size_t)numel / C;
  const int grid = row_grid(rows, 256 / (C / (dtype ? 8 : 4)));
  if (mask_coef && (y2 || outact)) return VQA_EARG;
  bn_dispatch<0, 1, 2>(dtype, bn_mask_mode(mask_coef != nullptr, y2), [&](auto t, auto m) {
    hipLaunchKernelGGL((bn_bwd_apply_kernel<BN_T, BN_M == 1, BN_M == 2, false>), dim3(grid), dim3(256), 0, st, (const BN_T*)dout, (const BN_T*)outact,
                       (const BN_T*)y, bc, (BN_T*)dy, (const BN_T*)y2, bc2, (BN_T*)dy2, rows, C, mask_coef);
  });
  VQA_LAUNCH_CHECK(); return VQA_OK;
}

}  // extern "C"
#undef BN_T
#undef BN_M
