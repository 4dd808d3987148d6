// Per-tensor statistics of a flat fp32 buffer (HipTrainer(monitor=...), kernels.tensor_stats): a deterministic SEGMENTED reduction,
// one result row per table row, in two launches and without float atomics.
//   d[i] = x[i]            (y == NULL)
//   d[i] = x[i] - y[i]     (one fp32 subtraction)
//   out[j] = { sum of d^2 over the finite d of row j (f32), max |d| over them (f32), #d that are NaN or +-inf (u32), #d == 0 (u32) }
// table: int64 rows {lo, hi, first_chunk}; [lo, hi) of the flat buffer, lo a multiple of 4, hi arbitrary; first_chunk = the number
// of chunks of the rows before it.  Chunk c of a row is [lo + c * CHUNK, min(hi, lo + (c + 1) * CHUNK)): chunks are anchored at the
// row's own lo, so what a row's workgroups read and the order they add in depend on (lo, hi) alone -- not on the grid, on P, or on
// where in the table the row stands.  Elements outside the rows (the layout's alignment padding, anything beyond) are never read.
//
// tensor_stats_chunk_kernel: one 256-thread workgroup per chunk (32 KB of x).  Thread t takes the float4 t + 256 k, k = 0 .. 7, of
//   the chunk -- a wave reads 1 KB per load instruction, and every load of a thread is issued before its first use -- and adds the
//   squares in element order, k ascending, with one fused multiply-add each; the last (hi - lo) mod 4 elements of a row go to
//   threads 0 .. 2 of its last chunk, one each, behind their float4s.  Then the wave butterfly (xor 32, 16, ... 1), then
//   (w0 + w1) + (w2 + w3) through LDS: one partial {sumsq, absmax, nonfinite, zeros} per chunk into scratch[4 * chunk].
// tensor_stats_fold_kernel: one wave per row folds the row's partials in ASCENDING chunk order, s = ((p0 + p1) + p2) + ...: the
//   wave loads 64 partials at a time, one per lane, and every lane adds them in lane order out of the registers (v_readlane).
//   absmax and the counts are exact in any order and take the butterfly.
//
// Rounding of sumsq.  A term goes through at most
//   N_add = T + 6 + 2 + chunks + 1,   T = min(32, 4 * ceil(min(numel, CHUNK) / 1024)) + (numel % 4 ? 1 : 0),  chunks = ceil(numel / CHUNK)
// roundings: T additions in its thread, 6 in the butterfly, 2 across the waves, one per chunk of its row in the fold, and 1 for its
// square (the fused multiply-add spares that one: the bound keeps it), + 1 in the pair form for the subtraction.  All terms are
// non-negative, so |sumsq - exact| <= N_add * 2^-24 * exact to first order (tests/test_gpu_tensor_stats_kernels.py computes N_add
// from numel and VQA_STATS_CHUNK).  A finite d whose square overflows gives +inf, as torch's norm does.
#include "common.h"

#ifndef VQA_STATS_CHUNK
#define VQA_STATS_CHUNK 8192          // include/vqa_hip.h (the sources do not include the public header; tests/test_tensor_stats_cpu.py compares)
#endif
#define VQA_STATS_MAX_ROWS 4096

namespace {

constexpr int STATS_THREADS = 256;
constexpr int STATS_VECS = VQA_STATS_CHUNK / (4 * STATS_THREADS);          // float4 per thread and chunk
static_assert(VQA_STATS_CHUNK % 1024 == 0 && STATS_VECS * 4 * STATS_THREADS == VQA_STATS_CHUNK, "a chunk is whole float4 rounds of the workgroup");

struct Stats {
  float s, mx; unsigned nf, z;
  __device__ __forceinline__ void add(float d) {
    const bool bad = (__float_as_uint(d) & 0x7f800000u) == 0x7f800000u;    // NaN or +-inf
    const float a = bad ? 0.f : fabsf(d);
    s = __builtin_fmaf(a, a, s);
    mx = fmaxf(mx, a);
    nf += bad ? 1u : 0u;
    z += d == 0.f ? 1u : 0u;                                               // (-0.0 == 0; a NaN is not)
  }
  __device__ __forceinline__ void add4(const f32x4& v) { add(v[0]); add(v[1]); add(v[2]); add(v[3]); }
};

__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o, 64);
  return v;
}

template <bool PAIR>
__global__ __launch_bounds__(STATS_THREADS) void tensor_stats_chunk_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                                           const long long* __restrict__ table, int P,
                                                                           u32x4* __restrict__ scratch) {
  __shared__ long long s_base;
  __shared__ int s_n;
  __shared__ float sh_s[4], sh_mx[4];
  __shared__ unsigned sh_nf[4], sh_z[4];
  const int t = threadIdx.x;
  const long long c = blockIdx.x;
  if (t == 0) { s_base = 0; s_n = 0; }
  __syncthreads();
  // the row of this chunk: every thread looks at its share of the table, one round of loads (exactly one row matches)
  for (int j = t; j < P; j += STATS_THREADS) {
    const long long lo = table[3 * j], hi = table[3 * j + 1], fc = table[3 * j + 2];
    if (c >= fc && c < fc + (hi - lo + VQA_STATS_CHUNK - 1) / VQA_STATS_CHUNK) {
      const long long base = lo + (c - fc) * VQA_STATS_CHUNK, left = hi - base;
      s_base = base;
      s_n = left < VQA_STATS_CHUNK ? (int)left : VQA_STATS_CHUNK;
    }
  }
  __syncthreads();
  const int n = s_n, n4 = n >> 2;
  const float* __restrict__ px = x + s_base;
  const float* __restrict__ py = PAIR ? y + s_base : nullptr;
  Stats a{0.f, 0.f, 0u, 0u};
  if (n4 > 0) {
    // One path for whole and cut chunks: a float4 past the end of a cut chunk is loaded from the chunk's LAST float4 instead (inside
    // the row, so nothing else is read) and not added -- the loads stay unconditional and all go out before the first addition.
    f32x4 vx[STATS_VECS], vy[STATS_VECS];
#pragma unroll
    for (int k = 0; k < STATS_VECS; ++k) {
      const int q = t + k * STATS_THREADS, qc = q < n4 ? q : n4 - 1;
      vx[k] = *reinterpret_cast<const f32x4*>(px + 4 * qc);
      if (PAIR) vy[k] = *reinterpret_cast<const f32x4*>(py + 4 * qc);
    }
#pragma unroll
    for (int k = 0; k < STATS_VECS; ++k)
      if (t + k * STATS_THREADS < n4) a.add4(PAIR ? vx[k] - vy[k] : vx[k]);
  }
  if (t < (n & 3)) {                                                       // the scalar tail: elements 4 * n4 + {0, 1, 2}
    const float dx = px[4 * n4 + t];
    a.add(PAIR ? dx - py[4 * n4 + t] : dx);
  }
  a.s = wave_sum(a.s); a.mx = wave_max(a.mx); a.nf = wave_sum_u32(a.nf); a.z = wave_sum_u32(a.z);
  if ((t & 63) == 0) { sh_s[t >> 6] = a.s; sh_mx[t >> 6] = a.mx; sh_nf[t >> 6] = a.nf; sh_z[t >> 6] = a.z; }
  __syncthreads();
  if (t == 0) {
    u32x4 o;
    o[0] = __float_as_uint((sh_s[0] + sh_s[1]) + (sh_s[2] + sh_s[3]));
    o[1] = __float_as_uint(fmaxf(fmaxf(sh_mx[0], sh_mx[1]), fmaxf(sh_mx[2], sh_mx[3])));
    o[2] = (sh_nf[0] + sh_nf[1]) + (sh_nf[2] + sh_nf[3]);
    o[3] = (sh_z[0] + sh_z[1]) + (sh_z[2] + sh_z[3]);
    scratch[c] = o;
  }
}

__global__ __launch_bounds__(STATS_THREADS) void tensor_stats_fold_kernel(const u32x4* __restrict__ scratch, const long long* __restrict__ table,
                                                                          int P, u32x4* __restrict__ out) {
  const int j = blockIdx.x * (STATS_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (j >= P) return;                                                      // (a whole wave leaves: the loop below is wave-uniform)
  const long long lo = table[3 * j], hi = table[3 * j + 1], fc = table[3 * j + 2];
  const long long nch = (hi - lo + VQA_STATS_CHUNK - 1) / VQA_STATS_CHUNK;
  const u32x4* __restrict__ p = scratch + fc;
  const u32x4 zero = {0u, 0u, 0u, 0u};                                     // (s + 0 keeps the bits of s >= +0: lanes past the end add nothing)
  float s = 0.f, mx = 0.f;
  unsigned nf = 0u, z = 0u;
  u32x4 cur = lane < nch ? p[lane] : zero;
  for (long long b = 0; b < nch; b += 64) {
    const u32x4 nxt = b + 64 + lane < nch ? p[b + 64 + lane] : zero;       // in flight while this batch is added
    mx = fmaxf(mx, __uint_as_float(cur[1])); nf += cur[2]; z += cur[3];
#pragma unroll
    for (int i = 0; i < 64; ++i) s += __uint_as_float((unsigned)__builtin_amdgcn_readlane((int)cur[0], i));
    cur = nxt;
  }
  mx = wave_max(mx); nf = wave_sum_u32(nf); z = wave_sum_u32(z);
  if (lane == 0) {
    u32x4 o;
    o[0] = __float_as_uint(s); o[1] = __float_as_uint(mx); o[2] = nf; o[3] = z;
    out[j] = o;
  }
}

}  // namespace

extern "C" {

int vqa_tensor_stats(const float* x, const float* y, const long long* table, int P, long long chunks, void* out, float* scratch,
                     hipStream_t st) {
  if (!x || !table || !out || !scratch || P < 1 || P > VQA_STATS_MAX_ROWS || chunks < P || chunks > 0x7fffffffll) return VQA_EARG;
  u32x4* part = reinterpret_cast<u32x4*>(scratch);
  if (y) hipLaunchKernelGGL(tensor_stats_chunk_kernel<true>, dim3((unsigned)chunks), dim3(STATS_THREADS), 0, st, x, y, table, P, part);
  else hipLaunchKernelGGL(tensor_stats_chunk_kernel<false>, dim3((unsigned)chunks), dim3(STATS_THREADS), 0, st, x, y, table, P, part);
  VQA_LAUNCH_CHECK();
  hipLaunchKernelGGL(tensor_stats_fold_kernel, dim3((unsigned)(P + 3) / 4), dim3(STATS_THREADS), 0, st, (const u32x4*)part, table, P,
                     reinterpret_cast<u32x4*>(out));
  VQA_LAUNCH_CHECK(); return VQA_OK;
}

}  // extern "C"
