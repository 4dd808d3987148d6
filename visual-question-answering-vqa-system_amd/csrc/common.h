// Shared device helpers for the gfx950 (MI355X, CDNA4) VQA kernels.  Wave = 64 lanes.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/vqa_hip.h"
#include <stddef.h>
#include <stdint.h>

#include <stdlib.h>

#include <atomic>
#include <mutex>

// Measurement / ablation switches (tile choices, and the VQA_*_DBG phase switches that give WRONG results on purpose) are
// environment variables only in builds made with -DVQA_ABLATION (tools/build_ablation.py makes its own libvqa_hip_ablation.so).
// The product library ignores the environment: every switch is its shipped default, folded at compile time.
#ifdef VQA_ABLATION
static inline int vqa_env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
#else
static inline int vqa_env_int(const char*, int dflt) { return dflt; }
#endif

#define VQA_OK 0
#define VQA_EARG 1000   // argument / shape error (never launches)

typedef uint16_t bf16_t;   // raw bfloat16 bits
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) short i16x4;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

__device__ __forceinline__ float bf2f(bf16_t v) { return __uint_as_float(((uint32_t)v) << 16); }
__device__ __forceinline__ bf16_t f2bf(float f) {   // RNE, NaN stays NaN (v_cvt_pk_bf16_f32)
  __bf16 b = (__bf16)f;
  return __builtin_bit_cast(bf16_t, b);
}
template <typename T> __device__ __forceinline__ float to_f(T v);
template <> __device__ __forceinline__ float to_f<float>(float v) { return v; }
template <> __device__ __forceinline__ float to_f<bf16_t>(bf16_t v) { return bf2f(v); }
template <typename T> __device__ __forceinline__ T from_f(float v);
template <> __device__ __forceinline__ float from_f<float>(float v) { return v; }
template <> __device__ __forceinline__ bf16_t from_f<bf16_t>(float v) { return f2bf(v); }

// 16-byte vector of T (4 floats or 8 bf16) with element access as float.
template <typename T> struct Vec16;
template <> struct Vec16<float> {
  static constexpr int N = 4;
  u32x4 raw;
  __device__ __forceinline__ float get(int i) const { return __uint_as_float(raw[i]); }
  __device__ __forceinline__ void set(int i, float v) { raw[i] = __float_as_uint(v); }
};
template <> struct Vec16<bf16_t> {
  static constexpr int N = 8;
  u32x4 raw;
  __device__ __forceinline__ float get(int i) const {
    uint32_t w = raw[i >> 1];
    return __uint_as_float((i & 1) ? (w & 0xffff0000u) : (w << 16));
  }
  __device__ __forceinline__ void set(int i, float v) {
    uint32_t b = f2bf(v);
    uint32_t w = raw[i >> 1];
    raw[i >> 1] = (i & 1) ? ((w & 0x0000ffffu) | (b << 16)) : ((w & 0xffff0000u) | b);
  }
};
template <typename T> __device__ __forceinline__ Vec16<T> ldg16(const T* p) {
  Vec16<T> v; v.raw = *reinterpret_cast<const u32x4*>(p); return v;
}
template <typename T> __device__ __forceinline__ void stg16(T* p, const Vec16<T>& v) {
  *reinterpret_cast<u32x4*>(p) = v.raw;
}
template <typename T> __device__ __forceinline__ Vec16<T> zero16() {
  Vec16<T> v; v.raw = u32x4{0u, 0u, 0u, 0u}; return v;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// Counter-based dropout RNG: keep(seed, idx) is a pure function so backward regenerates the mask.
__device__ __forceinline__ uint32_t mix32(uint32_t x) {
  x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16; return x;
}
// Fast form for tensors below 2^32 elements (every tensor of this model): the seed-only half of the hash is computed once per
// kernel (drop_key) and each element costs ONE mix32 instead of two; bit-identical to drop_keep for idx < 2^32.
__device__ __forceinline__ uint32_t drop_key(uint64_t seed) { return mix32((uint32_t)seed) ^ (uint32_t)(seed >> 32) * 0x9E3779B9u; }
__device__ __forceinline__ bool drop_keep32(uint32_t key, uint32_t idx, float p) {
  const uint32_t h = mix32(idx ^ key);
  return (float)(h >> 8) * (1.0f / 16777216.0f) >= p;
}
// A seed word is self-describing.  Bit 63 clear: the seed itself (rank << 44 | step << 12 | site: the rank sits at bit 44, so a plain
// seed never reaches bit 63).  Bit 63 set: bits 0-47 hold the device address of vqa_step_state::seed_step (rank << 44 | step << 12 of
// the step being run, written by vqa_step_state_set) and bits 48-59 the site; the seed is that word | site.  A captured train step
// carries such words, so every replay draws the masks of ITS step.  One uniform 8-byte read: call it once at the top of a kernel,
// never per element (drop_key / drop_keep take the resolved value).
#define VQA_SEED_INDIRECT (1ull << 63)
__device__ __forceinline__ uint64_t drop_resolve(uint64_t seed) {
  if (!(seed & VQA_SEED_INDIRECT)) return seed;
  const unsigned long long* word = reinterpret_cast<const unsigned long long*>((uintptr_t)(seed & 0xFFFFFFFFFFFFull));
  return (uint64_t)*word | ((seed >> 48) & 0xFFFull);
}
__device__ __forceinline__ bool drop_keep(uint64_t seed, uint64_t idx, float p) {
  uint32_t h = mix32((uint32_t)idx ^ mix32((uint32_t)(idx >> 32) + (uint32_t)seed) ^ (uint32_t)(seed >> 32) * 0x9E3779B9u);
  return (float)(h >> 8) * (1.0f / 16777216.0f) >= p;
}

// ------------------------------------------------------------------------------------------------------------------
// Order-independent accumulation of fp32 partial sums across workgroups: FIXED POINT in 64-bit integer atomics.  Integer addition
// commutes, so the total is bit-identical whatever order the workgroups arrive in (float atomics are not: the train step is
// bit-reproducible, tests/test_gpu_reproducible.py), and the consumer kernel can read the finished sums in its prologue -- no
// slab, no separate finalize launch between producer and consumer (60 such launches sat on the critical path of a train step).
//
// A partial (one workgroup's fp32 sum v) is split EXACTLY into  v = hi/2^4 + lo,  hi = rint(16 v) an integer, |lo| <= 2^-5, and the
// two halves go to two integer planes: hi as it is, lo scaled by 2^50.  Range and resolution are therefore independent:
//   |v| < 2^41 (2.2e12) per partial, resolution 2^-50 (8.9e-16) -- both BatchNorm statistics (sum y, sum y^2) and the BatchNorm
//   backward sums (sum g, sum g*xhat; under GradScaler these are multiplied by a loss scale that doubles every 2000 clean steps,
//   training/train.py:179-195) fit with one format.
// The TOTAL cannot wrap: with at most VQA_ACC_MAX_PARTS = 2^17 partials per sum (the launchers refuse larger grids) the hi plane
// stays below 2^45 * 2^17 = 2^62 and the lo plane below 2^45 * 2^17 as well, replicas included.  (Round 3 range-checked only the
// partial: ~96 partials just under the old 2^22 backward limit wrapped the int64 total silently -- finite and wrong.)
// A partial outside the range, or NaN / inf, raises the flag word; the consumer then turns the statistics into NaN (loud: under AMP
// the GradScaler sees non-finite gradients, skips the step and backs the scale off, as it would for an fp16 overflow).
// ------------------------------------------------------------------------------------------------------------------
// Replicas: a sum lives in R copies (producer workgroup w adds to copy w % R, the consumer adds the copies as integers) because
// atomics on ONE address are serialised at ~21 ns each on MI355X (tools/atomic_bench.hip: 768 workgroups x 256 addresses 57 us with
// one copy, 4 us with eight); R = 512 / C clamped to 1..8 keeps R*C constant, so a consumer prologue reads the same few KB whatever C.
//   layout (n = R*K*C):  hi plane acc[(r*K + k)*C + c] | flag acc[n] | lo plane acc[n + 1 + (r*K + k)*C + c];
//   vqa_bn_acc_words(K, C) = 2n + 1 rounded up to even, caller-zeroed.
static inline __host__ __device__ int acc_replicas(int C) { const int r = 512 / (C > 0 ? C : 1); return r < 1 ? 1 : (r > 8 ? 8 : r); }
#define VQA_ACC_HI_SHIFT 4
#define VQA_ACC_LO_SHIFT 50
#define VQA_ACC_MAX_PARTS (1 << 17)
#define VQA_ACC_LIMIT_LOG2 (62 - VQA_ACC_HI_SHIFT - 17)       // 41
// idx = (r*K + k)*C + c,  n = R*K*C
__device__ __forceinline__ void acc_add_fixed(unsigned long long* acc, size_t n, size_t idx, float v) {
  constexpr float lim = (float)(1ull << VQA_ACC_LIMIT_LOG2), hs = (float)(1 << VQA_ACC_HI_SHIFT), lscale = (float)(1ull << VQA_ACC_LO_SHIFT);
  if (fabsf(v) < lim) {                                                          // (NaN fails the comparison too)
    const float hi = rintf(v * hs);                                              // integer, |hi| < 2^45: the conversion below is exact
    const float lo = __builtin_fmaf(hi, -1.f / hs, v);                           // exact: a multiple of ulp(v) no larger than 2^-5
    atomicAdd(acc + idx, (unsigned long long)(long long)hi);
    if (lo != 0.f) atomicAdd(acc + n + 1 + idx, (unsigned long long)__float2ll_rn(lo * lscale));
  } else atomicAdd(acc + n, 1ull);
}
// sum k of channel c over the R <= 8 replicas (integer addition: exact, order-free), as a double.  All loads are issued before
// the first add: a serial loop over a runtime R is a chain of dependent L2 latencies (24 of them cost a consumer 12 us).
__device__ __forceinline__ double acc_read_fixed(const unsigned long long* acc, int R, int K, int C, int k, int c) {
  const size_t n = (size_t)R * K * C;
  long long h[8], l[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const size_t i = ((size_t)r * K + k) * C + c;
    h[r] = r < R ? (long long)acc[i] : 0ll;
    l[r] = r < R ? (long long)acc[n + 1 + i] : 0ll;
  }
  const long long th = ((h[0] + h[1]) + (h[2] + h[3])) + ((h[4] + h[5]) + (h[6] + h[7]));
  const long long tl = ((l[0] + l[1]) + (l[2] + l[3])) + ((l[4] + l[5]) + (l[6] + l[7]));
  return (double)th * (1.0 / (double)(1 << VQA_ACC_HI_SHIFT)) + (double)tl * (1.0 / (double)(1ull << VQA_ACC_LO_SHIFT));
}
__device__ __forceinline__ bool acc_flagged(const unsigned long long* acc, int R, int K, int C) { return acc[(size_t)R * K * C] != 0; }

struct BnAcc {
  const unsigned long long* acc; const float* gamma; const float* beta; float* rm; float* rv; long long* nbt; float* coef;
};
// One evaluation per channel and workgroup (the results are shared through LDS), fp64 only for the cancellation-prone
// var = E[y^2] - mean^2; 1/count arrives precomputed and 1/sqrt is the fp32 hardware instruction -- a first version that divided
// and took square roots in fp64 in every thread cost 3x the streaming work of the kernel.
__device__ __forceinline__ void bn_acc_coef(const BnAcc& f, int C, int c, double inv_count, double unbias, float momentum, float eps, bool writer,
                                            float& sc, float& sh) {
  const int R = acc_replicas(C);
  const double s = acc_read_fixed(f.acc, R, 2, C, 0, c), q = acc_read_fixed(f.acc, R, 2, C, 1, c);
  double mean = s * inv_count;
  double var = q * inv_count - mean * mean;
  if (var < 0.0) var = 0.0;
  if (acc_flagged(f.acc, R, 2, C)) mean = __builtin_nan("");                 // a partial sum left the fixed-point range / was not finite
  const float invstd = rsqrtf((float)var + eps);
  sc = f.gamma[c] * invstd; sh = f.beta[c] - (float)mean * sc;
  if (writer) {
    f.coef[c] = sc; f.coef[C + c] = sh; f.coef[2 * C + c] = (float)mean; f.coef[3 * C + c] = invstd;
    if (f.rm) {
      f.rm[c] = (1.f - momentum) * f.rm[c] + momentum * (float)mean;
      f.rv[c] = (1.f - momentum) * f.rv[c] + momentum * (float)(var * unbias);
      if (c == 0 && f.nbt) *f.nbt += 1;
    }
  }
}

// include/vqa_hip.h (included above) is the one declaration of every entry and of the two device blocks: each source compiles against
// it, so a definition whose arguments disagree with it does not compile ("conflicting types"), and nothing is declared a second time here
// or in a source.  The assertions pin the layout the ctypes mirrors of stepgraph.py assume.
static_assert(sizeof(vqa_step_state) == 64 && alignof(vqa_step_state) == 16, "vqa_step_state: 52 bytes of fields in a 16-byte aligned block");
static_assert(offsetof(vqa_step_state, seed_step) == 8 && offsetof(vqa_step_state, lr) == 16 && offsetof(vqa_step_state, ema_warmup) == 48,
              "vqa_step_state: field order of include/vqa_hip.h");
static_assert(sizeof(vqa_group_hyper) == 128 && alignof(vqa_group_hyper) == 16 && offsetof(vqa_group_hyper, wd) == 64,
              "vqa_group_hyper: two arrays of 16 floats in a 16-byte aligned block");

#define VQA_LAUNCH_CHECK() do { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return (int)e_; } while (0)
// an entry's `int dtype` argument picks the launch: 0 = the fp32 instantiation (call_f), 1 = the bf16 one (call_b)
#define DT(call_f, call_b) do { if (dtype) { call_b; } else { call_f; } } while (0)

// The shape every kernel that gives a thread one 16-byte channel vector and a 256-thread workgroup whole rows asks for (BatchNorm, SE,
// spatial attention): C a positive multiple of the vector (8 bf16 | 4 fp32), at most 256 vectors, a count that divides 256.
static inline bool bn_vec_ok(int dtype, int C) { const int VEC = dtype ? 8 : 4; return C > 0 && !(C % VEC || C / VEC > 256 || 256 % (C / VEC)); }

// dst0[c] (c < n0) / dst1[c - n0] += sum over rows r < nrows of part[r * stride + c], rows in index order (fold_rows_kernel).  Defined in
// token_ops.hip, where the kernel lives: other translation units launch it through this, so its device code exists once.
void vqa_launch_fold(const float* part, int nrows, size_t stride, int ncols, float* dst0, int n0, float* dst1, hipStream_t st);

// ------------------------------------------------------------------------------------------------------------------
// Dynamic LDS above the default limit: every launch site calls vqa_ensure_lds(kernel, bytes) before its launch.  The largest size
// set so far is remembered per (kernel, device) in a fixed lock-free table, so the common case is one hipGetDevice and a few atomic
// loads; only a size larger than the recorded one takes the mutex and calls hipFuncSetAttribute, and under the mutex the recorded
// size only grows, so racing threads never leave a smaller limit set last.  (Table full or device index out of range: the
// attribute is set on every call, still correct.)  Returns the HIP error; launch sites keep VQA_LAUNCH_CHECK.
// ------------------------------------------------------------------------------------------------------------------
#define VQA_LDS_SLOTS 256
#define VQA_LDS_DEVICES 16
struct VqaLdsSlot { std::atomic<const void*> kernel; std::atomic<size_t> bytes[VQA_LDS_DEVICES]; };
inline VqaLdsSlot vqa_lds_slots[VQA_LDS_SLOTS];       // zero-initialised, shared by every translation unit of the library
inline std::mutex vqa_lds_mutex;

static inline VqaLdsSlot* vqa_lds_find(const void* kernel, bool insert) {
  const size_t h = (size_t)(reinterpret_cast<uintptr_t>(kernel) >> 4) % VQA_LDS_SLOTS;
  for (size_t i = 0; i < VQA_LDS_SLOTS; ++i) {
    VqaLdsSlot& s = vqa_lds_slots[(h + i) % VQA_LDS_SLOTS];
    const void* k = s.kernel.load(std::memory_order_acquire);
    if (k == kernel) return &s;
    if (!k) {                                          // slots are only ever claimed under the mutex (insert == true)
      if (insert) s.kernel.store(kernel, std::memory_order_release);
      return insert ? &s : nullptr;
    }
  }
  return nullptr;
}
static inline hipError_t vqa_ensure_lds(const void* kernel, size_t bytes) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  const bool cached = dev >= 0 && dev < VQA_LDS_DEVICES;
  if (cached) {
    const VqaLdsSlot* s = vqa_lds_find(kernel, false);
    if (s && s->bytes[dev].load(std::memory_order_acquire) >= bytes) return hipSuccess;
  }
  std::lock_guard<std::mutex> lock(vqa_lds_mutex);
  VqaLdsSlot* s = cached ? vqa_lds_find(kernel, true) : nullptr;
  if (s && s->bytes[dev].load(std::memory_order_relaxed) >= bytes) return hipSuccess;
  e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess && s) s->bytes[dev].store(bytes, std::memory_order_release);
  return e;
}
