// The optimizer tail for gfx950, over flat fp32 buffers: global L2 norm of the gradient, clip, AdamW (decoupled weight decay), the
// weight average (EMA) and the device step-state block of a captured step.
//   clip_grad_norm_ / AdamW   training/train.py:204-208, :127-132
// ONE AdamW: one prologue (adam_skipped, adam_t0, clip_coef, adam_step_at), one element update (adam_elem), two loops over them --
// flat (every element of the buffer) and ranges (a table of trainable ranges) -- each compiled with and without the weight average
// (EMA) and with its hyper-parameters from the kernel arguments (HyperArgs) or from the device step-state block (HyperState).  The
// eight entries that result give the same bits for the same inputs because they run the same statements, not because copies agree.
// Parameter groups (GROUPS) are a third flag of the ranges loop: each range then takes its learning rate and weight decay from a
// device block of per-group values (vqa_group_hyper) instead of the launch's; four more entries, the same statements again.
#include "common.h"

// Sum of a 256-thread block's values in a fixed order (wave sums, then (w0 + w1) + (w2 + w3)); thread 0 stores it to *dst.
__device__ __forceinline__ void block_sum_store(float s, float* dst) {
  __shared__ float sh[4];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) *dst = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
__device__ __forceinline__ float sumsq4(float4 v) { return v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w; }

// Deterministic two-stage sum of squares (replicas must compute bit-identical clip factors): per-block partials in a fixed
// slot each, then one block folds them in a fixed order.  out[0] = result, out[1 .. 1+blocks) = partials.
__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ g, size_t n, float* out) {
  float s = 0.f;
  const size_t nv = n / 4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (size_t)gridDim.x * blockDim.x)
    s += sumsq4(reinterpret_cast<const float4*>(g)[i]);
  if (blockIdx.x == 0) for (size_t i = nv * 4 + threadIdx.x; i < n; i += blockDim.x) s += g[i] * g[i];
  block_sum_store(s, out + 1 + blockIdx.x);
}
// GUARD (HipTrainer(nonfinite=...)): the block that folds the partials also judges the step, in the same launch.  The gradient is
// non-finite when its sum of squares is NaN or inf (exponent bits all ones: a NaN or inf element, or finite elements whose squares
// overflow -- torch's norm is inf there too).  word[0] becomes the EFFECTIVE skip word the AdamW kernels and adamw_lag_kernel read:
// the rows with an out-of-range target when there are any (such a step stays a bad-target step: bad[0] += rows, bad[1] += 1, the
// non-finite counters rest), else 1 for a non-finite gradient (nonfinite[0] += 1 -- the caller's to reset --, nonfinite[1] += 1,
// never reset), else 0 (no counter is written).  One thread, plain stores; the fold is the unguarded kernel's, statement for statement.
__device__ __forceinline__ bool nonfinite_f32(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }
struct SumsqGuard { const int* bad_step; int* word; int* bad; int* nonfinite; };
template <bool GUARD>
__global__ __launch_bounds__(256) void sumsq_final_kernel(float* out, int nparts, SumsqGuard gd) {
  float s = 0.f;
  for (int i = threadIdx.x; i < nparts; i += 256) s += out[1 + i];
  block_sum_store(s, out);
  if constexpr (GUARD) {
    if (threadIdx.x == 0) {                     // (the thread that stored out[0] reads it back)
      const int rows = gd.bad_step ? *gd.bad_step : 0;
      int w = rows;
      if (rows != 0) {
        if (gd.bad) { gd.bad[0] += rows; gd.bad[1] += 1; }
      } else if (nonfinite_f32(out[0])) {
        w = 1;
        gd.nonfinite[0] += 1; gd.nonfinite[1] += 1;
      }
      *gd.word = w;
    }
  }
}

// A table of TRAINABLE ranges (fine-tuning with frozen parameters, trainer.py): elements outside every range are never read or
// written.  table: int64 rows {lo, hi, pos, lag index} -- [lo, hi) of the flat buffer, pos = where the range starts in the
// concatenation of all ranges (ascending); lo, hi, pos multiples of 4 (the layout's 8-element slots), so every float4 lies inside one
// range.  Threads stride over that concatenation: the grid is sized to the trainable count, not to the buffer.
#define VQA_RANGES_MAX 512
__device__ __forceinline__ int range_of(const long long* __restrict__ pos, int R, long long e) {
  int lo = 0, hi = R - 1;                   // the last range whose pos <= e
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (pos[mid] <= e) lo = mid; else hi = mid - 1;
  }
  return lo;
}
// element e of the concatenation: its range r and its index in the flat buffer
__device__ __forceinline__ long long range_index(const long long* s_lo, const long long* s_pos, int R, long long e, int& r) {
  r = range_of(s_pos, R, e);
  return s_lo[r] + (e - s_pos[r]);
}
__global__ __launch_bounds__(256) void sumsq_ranges_kernel(const float* __restrict__ g, const long long* __restrict__ table, int R, long long n,
                                                           float* out) {
  __shared__ long long s_lo[VQA_RANGES_MAX], s_pos[VQA_RANGES_MAX];
  for (int r = threadIdx.x; r < R; r += blockDim.x) { s_lo[r] = table[4 * r]; s_pos[r] = table[4 * r + 2]; }
  __syncthreads();
  float s = 0.f;
  const long long nv = n / 4;
  for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < nv; q += (long long)gridDim.x * blockDim.x) {
    int r;
    s += sumsq4(*reinterpret_cast<const float4*>(g + range_index(s_lo, s_pos, R, 4 * q, r)));
  }
  block_sum_store(s, out + 1 + blockIdx.x);
}

// Exponential moving average of the weights: ema = d * ema + (1 - d) * p_new, fp32.  ONE expression for the fused AdamW variants and
// the stand-alone pass (the same p_new and ema give the same bits whichever launch computes them): 1 - d and its product with p are
// each rounded once, the sum is one fma; contraction is off so that no surrounding code can change that.
__device__ __forceinline__ float ema_blend(float e, float p, float d) {
#pragma clang fp contract(off)
  const float q = (1.f - d) * p;
  return __builtin_fmaf(d, e, q);
}
// decay of the update at Adam step t: the caller's decay, or with warm-up min(decay, (1 + t) / (10 + t)) -- 2/11 at the first
// applied step, within 1 % of 0.999 from t = 8981 on: the average forgets the initial weights quickly and settles at the decay
__device__ __forceinline__ float ema_decay_at(float decay, int warmup, long long t) {
  if (!warmup) return decay;
  return fminf(decay, (float)(1 + t) / (float)(10 + t));
}

// The by-value hyper-parameters of one AdamW launch.  A kernel gets them from a source it is templated on: HyperArgs carries them
// as kernel arguments; HyperState names the device step-state block (vqa_step_state, written by vqa_step_state_set right before a
// captured step is replayed) and reads it on the device when the kernel runs -- a captured graph replays with the block's values of
// that moment.
struct AdamHyper { float lr, b1, b2, eps, wd; long long calls; float max_norm, gscale, ema_decay; int ema_warmup; };
__device__ __forceinline__ AdamHyper adam_hyper_of(const vqa_step_state* __restrict__ st) {
  AdamHyper h;
  h.lr = st->lr; h.b1 = st->b1; h.b2 = st->b2; h.eps = st->eps; h.wd = st->wd; h.calls = st->calls;
  h.max_norm = st->max_norm; h.gscale = st->gscale; h.ema_decay = st->ema_decay; h.ema_warmup = st->ema_warmup;
  return h;
}
struct HyperArgs { AdamHyper h; __device__ __forceinline__ AdamHyper get() const { return h; } };
struct HyperState { const vqa_step_state* state; __device__ __forceinline__ AdamHyper get() const { return adam_hyper_of(state); } };

// skip[0] != 0 (rows with an out-of-range target in THIS step, summed over ranks): the reference raises before optimizer.step()
// (nn.CrossEntropyLoss, training/train.py:120,182-208) and leaves the model intact -- so does every AdamW kernel: it returns when
// this is true, parameters, both moments, the bf16 copy and the average untouched; skipped[0] += rows, skipped[1] += 1 (read by the
// host at its logging interval), skipped[2] += 1 (never reset: the device-side record of how many launches did NOT count as a step).
__device__ __forceinline__ bool adam_skipped(const int* __restrict__ skip, int* __restrict__ skipped) {
  if (!skip || *skip == 0) return false;
  if (skipped && blockIdx.x == 0 && threadIdx.x == 0) { skipped[0] += *skip; skipped[1] += 1; skipped[2] += 1; }
  return true;
}
// Adam's step number lives on the DEVICE: calls (the host's launch count, this one included) minus the launches skipped so far.
// skipped[2] is only written by a launch that skips, and such a launch reads it nowhere else: no race.  (Round 3 derived the bias
// corrections from a host counter that was repaired only at the caller's next check(): every step in between ran one step ahead.)
__device__ __forceinline__ long long adam_t0(long long calls, const int* __restrict__ skipped) {
  return calls - (skipped ? (long long)skipped[2] : 0ll);
}
// what multiplies a raw gradient: the loss scale's inverse, times clip_grad_norm_'s coefficient when the norm exceeds max_norm
__device__ __forceinline__ float clip_coef(const float* __restrict__ sumsq, float max_norm, float gscale) {
  float coef = gscale;
  if (sumsq && max_norm > 0.f) {
    const float norm = sqrtf(*sumsq) * gscale;
    const float c = max_norm / (norm + 1e-6f);
    if (c < 1.f) coef *= c;
  }
  return coef;
}
// the scalars that depend on the step number t: lr / bias correction 1, 1 / sqrt(bias correction 2), the average's decay
struct AdamStep { float step, rbc2, d; };
template <bool EMA>
__device__ __forceinline__ AdamStep adam_step_at(const AdamHyper& hy, float lr, long long t) {
  const float bc1 = (float)(1.0 - pow((double)hy.b1, (double)t)), bc2 = (float)(1.0 - pow((double)hy.b2, (double)t));
  AdamStep s;
  s.step = lr / bc1; s.rbc2 = 1.f / sqrtf(bc2);
  s.d = 0.f;
  if constexpr (EMA) s.d = ema_decay_at(hy.ema_decay, hy.ema_warmup, t);
  return s;
}
// one element: p, m, v in, p, m, v out; lr and wd are the element's own (the launch's, or its parameter group's)
__device__ __forceinline__ void adam_elem(float& p, float& m, float& v, float g, const AdamHyper& hy, float lr, float wd, float coef,
                                          float step, float rbc2) {
  const float b1 = hy.b1, b2 = hy.b2, eps = hy.eps;
  const float gr = g * coef;
  float pi = p * (1.f - lr * wd);
  const float mi = b1 * m + (1.f - b1) * gr;
  const float vi = b2 * v + (1.f - b2) * gr * gr;
  m = mi; v = vi;
  pi -= step * mi / (sqrtf(vi) * rbc2 + eps);
  p = pi;
}

// Flat: clip + AdamW over all n elements.  p_bf16 != nullptr: the bf16 working copy of the parameters (what the next forward's GEMMs
// read) is written here as well -- the separate cast launch over the flat buffer (116 MB of traffic, 34 us at the head of every
// step) is gone.  EMA: the average of the updated parameter, taken from the register that still holds it: 8 B per element on top of
// the 28 B, no second read of p.  A skipped launch does not advance t, so neither does the average's warm-up.
template <bool EMA, class Hyper>
__global__ void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, size_t n,
                             Hyper src, const float* __restrict__ sumsq, const int* __restrict__ skip, int* __restrict__ skipped,
                             bf16_t* __restrict__ p_bf16, float* __restrict__ ema) {
  const AdamHyper hy = src.get();
  if (adam_skipped(skip, skipped)) return;
  const AdamStep s = adam_step_at<EMA>(hy, hy.lr, adam_t0(hy.calls, skipped));
  const float coef = clip_coef(sumsq, hy.max_norm, hy.gscale);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float gi = g[i];
    float pi = p[i], mi = m[i], vi = v[i];
    adam_elem(pi, mi, vi, gi, hy, hy.lr, hy.wd, coef, s.step, s.rbc2);
    m[i] = mi; v[i] = vi; p[i] = pi;
    if (p_bf16) p_bf16[i] = f2bf(pi);
    if constexpr (EMA) ema[i] = ema_blend(ema[i], pi, s.d);
  }
}

// Ranges: the same over the table's ranges, one float4 per thread and trip.  Adam's step number of range r is
// calls - skipped[2] - lag[table[r].lag index], where lag[j] counts the applied steps during which parameter j was frozen
// (torch.optim.AdamW advances a parameter's `step` only when it has a gradient); every parameter inside one range shares its lag (the
// caller merges only such neighbours).  The average's warm-up of range r runs on that range's OWN step number (a parameter's average
// advances only while it trains), and `ema` is neither read nor written outside the ranges.
// GROUPS (parameter groups): range r belongs to group g = group_of_range[r] and is updated with lr * groups->lr_scale[g] and
// groups->wd[g] in the place of lr and wd -- two more per-range scalars next to the step's (4 KB of LDS on top of 12 - 14: still
// eight workgroups per CU).  The block is read on the device when the kernel runs, so a captured launch follows vqa_group_hyper_set.
// g is the caller's to keep in 0 ... 15; it is taken modulo 16, so no index reads outside the block.
template <bool EMA, class Hyper, bool GROUPS>
__global__ __launch_bounds__(256) void adamw_ranges_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, const long long* __restrict__ table, int R, long long n,
                                                           Hyper src, const float* __restrict__ sumsq, const int* __restrict__ skip,
                                                           int* __restrict__ skipped, const int* __restrict__ lag,
                                                           bf16_t* __restrict__ p_bf16, float* __restrict__ ema,
                                                           const int* __restrict__ group_of_range,
                                                           const vqa_group_hyper* __restrict__ groups) {
  const AdamHyper hy = src.get();
  if (adam_skipped(skip, skipped)) return;
  __shared__ long long s_lo[VQA_RANGES_MAX], s_pos[VQA_RANGES_MAX];
  __shared__ float s_step[VQA_RANGES_MAX], s_rbc2[VQA_RANGES_MAX];
  __shared__ float s_d[EMA ? VQA_RANGES_MAX : 1];          // (never referenced without EMA: takes no LDS then)
  __shared__ float s_lr[GROUPS ? VQA_RANGES_MAX : 1], s_wd[GROUPS ? VQA_RANGES_MAX : 1];     // (nor these without GROUPS)
  const long long t0 = adam_t0(hy.calls, skipped);
  for (int r = threadIdx.x; r < R; r += blockDim.x) {
    s_lo[r] = table[4 * r]; s_pos[r] = table[4 * r + 2];
    float lr_r = hy.lr;
    if constexpr (GROUPS) {
      const int gi = group_of_range[r] & (VQA_GROUPS_MAX - 1);
      lr_r = hy.lr * groups->lr_scale[gi];
      s_lr[r] = lr_r; s_wd[r] = groups->wd[gi];
    }
    const AdamStep s = adam_step_at<EMA>(hy, lr_r, t0 - (lag ? (long long)lag[table[4 * r + 3]] : 0ll));
    s_step[r] = s.step; s_rbc2[r] = s.rbc2;
    if constexpr (EMA) s_d[r] = s.d;
  }
  __syncthreads();
  const float coef = clip_coef(sumsq, hy.max_norm, hy.gscale);
  const long long nv = n / 4;
  for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < nv; q += (long long)gridDim.x * blockDim.x) {
    int r;
    const long long i = range_index(s_lo, s_pos, R, 4 * q, r);
    const float step = s_step[r], rbc2 = s_rbc2[r];
    float lr = hy.lr, wd = hy.wd;
    if constexpr (GROUPS) { lr = s_lr[r]; wd = s_wd[r]; }
    const float4 g4 = *reinterpret_cast<const float4*>(g + i);
    float4 p4 = *reinterpret_cast<const float4*>(p + i);
    float4 m4 = *reinterpret_cast<const float4*>(m + i);
    float4 v4 = *reinterpret_cast<const float4*>(v + i);
    float4 e4;
    float d = 0.f;
    if constexpr (EMA) { e4 = *reinterpret_cast<const float4*>(ema + i); d = s_d[r]; }
    float* pp = &p4.x; float* mm = &m4.x; float* vv = &v4.x; const float* gg = &g4.x; float* ee = &e4.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      adam_elem(pp[k], mm[k], vv[k], gg[k], hy, lr, wd, coef, step, rbc2);
      if constexpr (EMA) ee[k] = ema_blend(ee[k], pp[k], d);
    }
    *reinterpret_cast<float4*>(p + i) = p4;
    *reinterpret_cast<float4*>(m + i) = m4;
    *reinterpret_cast<float4*>(v + i) = v4;
    if constexpr (EMA) *reinterpret_cast<float4*>(ema + i) = e4;
    if (p_bf16) {
      uint2 w;
      w.x = (uint32_t)f2bf(p4.x) | ((uint32_t)f2bf(p4.y) << 16);
      w.y = (uint32_t)f2bf(p4.z) | ((uint32_t)f2bf(p4.w) << 16);
      *reinterpret_cast<uint2*>(p_bf16 + i) = w;
    }
  }
}
// after an applied step: lag[frozen[k]] += 1 (one thread per frozen parameter; runs behind adamw_ranges_kernel on the same stream)
__global__ void adamw_lag_kernel(int* __restrict__ lag, const int* __restrict__ frozen, int nf, const int* __restrict__ skip) {
  if (skip && *skip != 0) return;
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < nf; k += gridDim.x * blockDim.x) lag[frozen[k]] += 1;
}

// The BatchNorm running buffers of a guarded step: by the time the gradient is judged the forward has overwritten them, so they are
// copied into one flat scratch ahead of the forward (save) and copied back behind the guarded norm when the effective skip word is
// set (restore; word == nullptr: save).  table: int64 rows {device address, 32-bit words, word offset into the scratch}, one workgroup
// per row; the buffers are fp32 or int64, so every size is whole words and every address 4-byte aligned.
__global__ __launch_bounds__(256) void buffers_copy_kernel(const long long* __restrict__ table, uint32_t* __restrict__ scratch,
                                                           const int* __restrict__ word) {
  if (word && *word == 0) return;
  const long long* row = table + 3 * (size_t)blockIdx.x;
  uint32_t* buf = reinterpret_cast<uint32_t*>((uintptr_t)row[0]);
  const long long nw = row[1];
  uint32_t* sc = scratch + row[2];
  if (word) { for (long long i = threadIdx.x; i < nw; i += 256) buf[i] = sc[i]; }
  else      { for (long long i = threadIdx.x; i < nw; i += 256) sc[i] = buf[i]; }
}
// Non-finite elements of the flat gradient per parameter: table = int64 rows {lo, hi} of P parameters (the padding behind hi belongs
// to no row), counts[P] += (integer atomics: exact whatever the order).  grid (P, NONFINITE_SCAN_SLICES).
constexpr int NONFINITE_SCAN_SLICES = 16;
__global__ __launch_bounds__(256) void nonfinite_scan_kernel(const float* __restrict__ g, const long long* __restrict__ table,
                                                             int* __restrict__ counts) {
  const long long lo = table[2 * (size_t)blockIdx.x], hi = table[2 * (size_t)blockIdx.x + 1];
  int c = 0;
  for (long long i = lo + (long long)blockIdx.y * 256 + threadIdx.x; i < hi; i += (long long)gridDim.y * 256) c += nonfinite_f32(g[i]) ? 1 : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(counts + blockIdx.x, c);
}

// One thread writes the step-state block (plain stores): launched eagerly on the stream right before a captured step is replayed; the
// values travel as kernel arguments, which the runtime copies at launch.
__global__ void step_state_set_kernel(vqa_step_state* state, long long calls, unsigned long long seed_step, float lr, float b1, float b2,
                                      float eps, float wd, float max_norm, float gscale, float ema_decay, int ema_warmup) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    state->calls = calls; state->seed_step = seed_step;
    state->lr = lr; state->b1 = b1; state->b2 = b2; state->eps = eps; state->wd = wd;
    state->max_norm = max_norm; state->gscale = gscale; state->ema_decay = ema_decay; state->ema_warmup = ema_warmup;
  }
}
// One thread writes the parameter groups' block, the same way: the 32 floats travel by value in the launch's arguments.
struct GroupHyperArg { float4 q[8]; };
__global__ void group_hyper_set_kernel(vqa_group_hyper* block, GroupHyperArg a) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 8; ++k) reinterpret_cast<float4*>(block)[k] = a.q[k];
  }
}
// The average as a pass of its own over a flat buffer (torch.optim loops: dropin/utils/ema.py): 12 B per element.  nv float4 groups
// (0 when a pointer is not 16-byte aligned), then the scalar rest.
__global__ __launch_bounds__(256) void ema_update_kernel(float* __restrict__ ema, const float* __restrict__ p, long long n, long long nv, float d) {
  const long long stride = (long long)gridDim.x * blockDim.x, i0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (long long q = i0; q < nv; q += stride) {
    const float4 p4 = reinterpret_cast<const float4*>(p)[q];
    float4 e4 = reinterpret_cast<float4*>(ema)[q];
    e4.x = ema_blend(e4.x, p4.x, d); e4.y = ema_blend(e4.y, p4.y, d); e4.z = ema_blend(e4.z, p4.z, d); e4.w = ema_blend(e4.w, p4.w, d);
    reinterpret_cast<float4*>(ema)[q] = e4;
  }
  for (long long i = 4 * nv + i0; i < n; i += stride) ema[i] = ema_blend(ema[i], p[i], d);
}

// ---------------------------------------------------------------------------------------------
// ceil(work / 256) blocks of 256 threads, clamped to [1, cap]
static inline unsigned blocks_of(size_t work, size_t cap) {
  size_t blocks = (work + 255) / 256; if (blocks > cap) blocks = cap; if (blocks < 1) blocks = 1;
  return (unsigned)blocks;
}
static inline bool ranges_args_ok(int R, long long n, int nf, const int* lag, const int* frozen) {
  return !(R < 0 || R > VQA_RANGES_MAX || n < 0 || n % 4 || (R == 0 && n != 0) || nf < 0 || (nf > 0 && (!lag || !frozen)));
}
static inline bool ema_decay_ok(float d) { return d >= 0.f && d <= 1.f; }        // (NaN fails both comparisons)
static inline bool state_ok(const void* state) { return state && !((uintptr_t)state & 15); }
static inline bool group_value_ok(float x) { return x >= 0.f && x <= 3.402823466e38f; }   // finite and not negative (NaN fails both)
static inline bool groups_ok(const int* group_of_range, const vqa_group_hyper* groups) { return group_of_range && state_ok(groups); }
static inline HyperArgs hyper_args(float lr, float b1, float b2, float eps, float wd, long long calls, float max_norm, float gscale,
                                   float ema_decay = 0.f, int ema_warmup = 0) {
  return HyperArgs{AdamHyper{lr, b1, b2, eps, wd, calls, max_norm, gscale, ema_decay, ema_warmup}};
}

// The two launchers behind the eight AdamW entries (arguments already checked by the entry).
template <bool EMA, class Hyper>
static int launch_adamw(float* p, const float* g, float* m, float* v, long long n, Hyper src, const float* sumsq, const int* skip, int* skipped,
                        void* p_bf16, float* ema, hipStream_t st) {
  hipLaunchKernelGGL((adamw_kernel<EMA, Hyper>), dim3(blocks_of((size_t)n, 4096)), dim3(256), 0, st, p, g, m, v, (size_t)n, src, sumsq, skip,
                     skipped, (bf16_t*)p_bf16, ema);
  VQA_LAUNCH_CHECK(); return VQA_OK;
}
template <bool EMA, bool GROUPS = false, class Hyper>
static int launch_adamw_ranges(float* p, const float* g, float* m, float* v, const long long* table, int R, long long n, Hyper src,
                               const float* sumsq, const int* skip, int* skipped, int* lag, const int* frozen, int nf, void* p_bf16,
                               float* ema, hipStream_t st, const int* group_of_range = nullptr, const vqa_group_hyper* groups = nullptr) {
  hipLaunchKernelGGL((adamw_ranges_kernel<EMA, Hyper, GROUPS>), dim3(blocks_of((size_t)n / 4, 4096)), dim3(256), 0, st, p, g, m, v, table, R,
                     n, src, sumsq, skip, skipped, (const int*)lag, (bf16_t*)p_bf16, ema, group_of_range, groups);
  if (nf > 0) hipLaunchKernelGGL(adamw_lag_kernel, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, st, lag, frozen, nf, skip);
  VQA_LAUNCH_CHECK(); return VQA_OK;
}

extern "C" {

int vqa_sumsq(const float* g, long long n, float* out, hipStream_t st) {
  const unsigned blocks = blocks_of((size_t)n / 4, 2048);
  hipLaunchKernelGGL(sumsq_kernel, dim3(blocks), dim3(256), 0, st, g, (size_t)n, out);
  hipLaunchKernelGGL(sumsq_final_kernel<false>, dim3(1), dim3(256), 0, st, out, (int)blocks, SumsqGuard{});
  VQA_LAUNCH_CHECK(); return VQA_OK;
}
int vqa_sumsq_ranges(const float* g, const long long* table, int R, long long n, float* out, hipStream_t st) {
  if (!ranges_args_ok(R, n, 0, nullptr, nullptr)) return VQA_EARG;
  const unsigned blocks = blocks_of((size_t)n / 4, 2048);
  hipLaunchKernelGGL(sumsq_ranges_kernel, dim3(blocks), dim3(256), 0, st, g, table, R, n, out);
  hipLaunchKernelGGL(sumsq_final_kernel<false>, dim3(1), dim3(256), 0, st, out, (int)blocks, SumsqGuard{});
  VQA_LAUNCH_CHECK(); return VQA_OK;
}
// The two norms with the non-finite guard in their fold block (same partial kernels, same grids, same fold: out[] has the same bits).
int vqa_sumsq_guard(const float* g, long long n, float* out, const int* bad_step, int* word, int* bad, int* nonfinite, hipStream_t st) {
  if (!g || !out || n < 0 || !word || !nonfinite) return VQA_EARG;
  const unsigned blocks = blocks_of((size_t)n / 4, 2048);
  hipLaunchKernelGGL(sumsq_kernel, dim3(blocks), dim3(256), 0, st, g, (size_t)n, out);
  hipLaunchKernelGGL(sumsq_final_kernel<true>, dim3(1), dim3(256), 0, st, out, (int)blocks, SumsqGuard{bad_step, word, bad, nonfinite});
  VQA_LAUNCH_CHECK(); return VQA_OK;
}
int vqa_sumsq_ranges_guard(const float* g, const long long* table, int R, long long n, float* out, const int* bad_step, int* word, int* bad,
                           int* nonfinite, hipStream_t st) {
  if (!g || !out || !table || !word || !nonfinite || !ranges_args_ok(R, n, 0, nullptr, nullptr)) return VQA_EARG;
  const unsigned blocks = blocks_of((size_t)n / 4, 2048);
  hipLaunchKernelGGL(sumsq_ranges_kernel, dim3(blocks), dim3(256), 0, st, g, table, R, n, out);
  hipLaunchKernelGGL(sumsq_final_kernel<true>, dim3(1), dim3(256), 0, st, out, (int)blocks, SumsqGuard{bad_step, word, bad, nonfinite});
  VQA_LAUNCH_CHECK(); return VQA_OK;
}
int vqa_buffers_save(const long long* table, int rows, void* scratch, hipStream_t st) {
  if (!table || !scratch || rows < 1 || rows > 65535) return VQA_EARG;
  hipLaunchKernelGGL(buffers_copy_kernel, dim3((unsigned)rows), dim3(256), 0, st, table, (uint32_t*)scratch, (const int*)nullptr);
  VQA_LAUNCH_CHECK(); return VQA_OK;
}
int vqa_buffers_restore(const long long* table, int rows, void* scratch, const int* word, hipStream_t st) {
  if (!table || !scratch || !word || rows < 1 || rows > 65535) return VQA_EARG;
  hipLaunchKernelGGL(buffers_copy_kernel, dim3((unsigned)rows), dim3(256), 0, st, table, (uint32_t*)scratch, word);
  VQA_LAUNCH_CHECK(); return VQA_OK;
}
int vqa_nonfinite_scan(const float* g, const long long* table, int P, int* counts, hipStream_t st) {
  if (!g || !table || !counts || P < 1 || P > (1 << 20)) return VQA_EARG;
  hipLaunchKernelGGL(nonfinite_scan_kernel, dim3((unsigned)P, NONFINITE_SCAN_SLICES), dim3(256), 0, st, g, table, counts);
  VQA_LAUNCH_CHECK(); return VQA_OK;
}

// clip + AdamW: flat / over a range table, without / with the weight average in the same launch.
int vqa_adamw(float* p, const float* g, float* m, float* v, long long n, float lr, float b1, float b2, float eps, float wd,
              long long calls, const float* sumsq, float max_norm, float gscale, const int* skip, int* skipped, void* p_bf16, hipStream_t st) {
  if (calls < 1) return VQA_EARG;
  return launch_adamw<false>(p, g, m, v, n, hyper_args(lr, b1, b2, eps, wd, calls, max_norm, gscale), sumsq, skip, skipped, p_bf16, nullptr, st);
}
int vqa_adamw_ema(float* p, const float* g, float* m, float* v, long long n, float lr, float b1, float b2, float eps, float wd,
                  long long calls, const float* sumsq, float max_norm, float gscale, const int* skip, int* skipped, void* p_bf16,
                  float* ema, float ema_decay, int ema_warmup, hipStream_t st) {
  if (calls < 1 || n < 0 || !ema || !ema_decay_ok(ema_decay)) return VQA_EARG;
  return launch_adamw<true>(p, g, m, v, n, hyper_args(lr, b1, b2, eps, wd, calls, max_norm, gscale, ema_decay, ema_warmup), sumsq, skip,
                            skipped, p_bf16, ema, st);
}
int vqa_adamw_ranges(float* p, const float* g, float* m, float* v, const long long* table, int R, long long n, float lr, float b1, float b2,
                     float eps, float wd, long long calls, const float* sumsq, float max_norm, float gscale, const int* skip, int* skipped,
                     int* lag, const int* frozen, int nf, void* p_bf16, hipStream_t st) {
  if (calls < 1 || !ranges_args_ok(R, n, nf, lag, frozen)) return VQA_EARG;
  return launch_adamw_ranges<false>(p, g, m, v, table, R, n, hyper_args(lr, b1, b2, eps, wd, calls, max_norm, gscale), sumsq, skip, skipped,
                                    lag, frozen, nf, p_bf16, nullptr, st);
}
int vqa_adamw_ranges_ema(float* p, const float* g, float* m, float* v, const long long* table, int R, long long n, float lr, float b1, float b2,
                         float eps, float wd, long long calls, const float* sumsq, float max_norm, float gscale, const int* skip, int* skipped,
                         int* lag, const int* frozen, int nf, void* p_bf16, float* ema, float ema_decay, int ema_warmup, hipStream_t st) {
  if (calls < 1 || !ranges_args_ok(R, n, nf, lag, frozen)) return VQA_EARG;
  if (!ema || !ema_decay_ok(ema_decay)) return VQA_EARG;
  return launch_adamw_ranges<true>(p, g, m, v, table, R, n, hyper_args(lr, b1, b2, eps, wd, calls, max_norm, gscale, ema_decay, ema_warmup),
                                   sumsq, skip, skipped, lag, frozen, nf, p_bf16, ema, st);
}

// The same four with their by-value hyper-parameters read from the device step-state block (same grids, same kernels' bodies).
int vqa_step_state_set(vqa_step_state* state, long long calls, unsigned long long seed_step, float lr, float b1, float b2, float eps,
                       float wd, float max_norm, float gscale, float ema_decay, int ema_warmup, hipStream_t st) {
  if (!state_ok(state) || calls < 1 || (seed_step & (VQA_SEED_INDIRECT | 0xFFFull))) return VQA_EARG;
  hipLaunchKernelGGL(step_state_set_kernel, dim3(1), dim3(1), 0, st, state, calls, seed_step, lr, b1, b2, eps, wd, max_norm, gscale, ema_decay,
                     ema_warmup);
  VQA_LAUNCH_CHECK(); return VQA_OK;
}
int vqa_adamw_dev(float* p, const float* g, float* m, float* v, long long n, const vqa_step_state* state, const float* sumsq,
                  const int* skip, int* skipped, void* p_bf16, hipStream_t st) {
  if (!state_ok(state) || n < 0) return VQA_EARG;
  return launch_adamw<false>(p, g, m, v, n, HyperState{state}, sumsq, skip, skipped, p_bf16, nullptr, st);
}
int vqa_adamw_ema_dev(float* p, const float* g, float* m, float* v, long long n, const vqa_step_state* state, const float* sumsq,
                      const int* skip, int* skipped, void* p_bf16, float* ema, hipStream_t st) {
  if (!state_ok(state) || n < 0 || !ema) return VQA_EARG;
  return launch_adamw<true>(p, g, m, v, n, HyperState{state}, sumsq, skip, skipped, p_bf16, ema, st);
}
int vqa_adamw_ranges_dev(float* p, const float* g, float* m, float* v, const long long* table, int R, long long n,
                         const vqa_step_state* state, const float* sumsq, const int* skip, int* skipped, int* lag, const int* frozen, int nf,
                         void* p_bf16, hipStream_t st) {
  if (!state_ok(state) || !ranges_args_ok(R, n, nf, lag, frozen)) return VQA_EARG;
  return launch_adamw_ranges<false>(p, g, m, v, table, R, n, HyperState{state}, sumsq, skip, skipped, lag, frozen, nf, p_bf16, nullptr, st);
}
int vqa_adamw_ranges_ema_dev(float* p, const float* g, float* m, float* v, const long long* table, int R, long long n,
                             const vqa_step_state* state, const float* sumsq, const int* skip, int* skipped, int* lag, const int* frozen,
                             int nf, void* p_bf16, float* ema, hipStream_t st) {
  if (!state_ok(state) || !ranges_args_ok(R, n, nf, lag, frozen)) return VQA_EARG;
  if (!ema) return VQA_EARG;
  return launch_adamw_ranges<true>(p, g, m, v, table, R, n, HyperState{state}, sumsq, skip, skipped, lag, frozen, nf, p_bf16, ema, st);
}

// Parameter groups: the block of per-group values, and the four range entries that read it on the device (the same launcher, GROUPS on).
int vqa_group_hyper_set(vqa_group_hyper* block, int G, const float* lr_scale, const float* wd, hipStream_t st) {
  if (!state_ok(block) || G < 1 || G > VQA_GROUPS_MAX || !lr_scale || !wd) return VQA_EARG;
  GroupHyperArg a = {};
  float* f = &a.q[0].x;
  for (int k = 0; k < G; ++k) {
    if (!group_value_ok(lr_scale[k]) || !group_value_ok(wd[k])) return VQA_EARG;
    f[k] = lr_scale[k]; f[VQA_GROUPS_MAX + k] = wd[k];
  }
  hipLaunchKernelGGL(group_hyper_set_kernel, dim3(1), dim3(1), 0, st, block, a);
  VQA_LAUNCH_CHECK(); return VQA_OK;
}
int vqa_adamw_groups(float* p, const float* g, float* m, float* v, const long long* table, int R, long long n, float lr, float b1, float b2,
                     float eps, float wd, long long calls, const float* sumsq, float max_norm, float gscale, const int* skip, int* skipped,
                     int* lag, const int* frozen, int nf, void* p_bf16, const int* group_of_range, const vqa_group_hyper* groups,
                     hipStream_t st) {
  if (calls < 1 || !ranges_args_ok(R, n, nf, lag, frozen) || !groups_ok(group_of_range, groups)) return VQA_EARG;
  return launch_adamw_ranges<false, true>(p, g, m, v, table, R, n, hyper_args(lr, b1, b2, eps, wd, calls, max_norm, gscale), sumsq, skip,
                                          skipped, lag, frozen, nf, p_bf16, nullptr, st, group_of_range, groups);
}
int vqa_adamw_groups_ema(float* p, const float* g, float* m, float* v, const long long* table, int R, long long n, float lr, float b1, float b2,
                         float eps, float wd, long long calls, const float* sumsq, float max_norm, float gscale, const int* skip, int* skipped,
                         int* lag, const int* frozen, int nf, void* p_bf16, float* ema, float ema_decay, int ema_warmup,
                         const int* group_of_range, const vqa_group_hyper* groups, hipStream_t st) {
  if (calls < 1 || !ranges_args_ok(R, n, nf, lag, frozen) || !groups_ok(group_of_range, groups)) return VQA_EARG;
  if (!ema || !ema_decay_ok(ema_decay)) return VQA_EARG;
  return launch_adamw_ranges<true, true>(p, g, m, v, table, R, n, hyper_args(lr, b1, b2, eps, wd, calls, max_norm, gscale, ema_decay, ema_warmup),
                                         sumsq, skip, skipped, lag, frozen, nf, p_bf16, ema, st, group_of_range, groups);
}
int vqa_adamw_groups_dev(float* p, const float* g, float* m, float* v, const long long* table, int R, long long n,
                         const vqa_step_state* state, const float* sumsq, const int* skip, int* skipped, int* lag, const int* frozen, int nf,
                         void* p_bf16, const int* group_of_range, const vqa_group_hyper* groups, hipStream_t st) {
  if (!state_ok(state) || !ranges_args_ok(R, n, nf, lag, frozen) || !groups_ok(group_of_range, groups)) return VQA_EARG;
  return launch_adamw_ranges<false, true>(p, g, m, v, table, R, n, HyperState{state}, sumsq, skip, skipped, lag, frozen, nf, p_bf16, nullptr,
                                          st, group_of_range, groups);
}
int vqa_adamw_groups_ema_dev(float* p, const float* g, float* m, float* v, const long long* table, int R, long long n,
                             const vqa_step_state* state, const float* sumsq, const int* skip, int* skipped, int* lag, const int* frozen,
                             int nf, void* p_bf16, float* ema, const int* group_of_range, const vqa_group_hyper* groups, hipStream_t st) {
  if (!state_ok(state) || !ranges_args_ok(R, n, nf, lag, frozen) || !groups_ok(group_of_range, groups)) return VQA_EARG;
  if (!ema) return VQA_EARG;
  return launch_adamw_ranges<true, true>(p, g, m, v, table, R, n, HyperState{state}, sumsq, skip, skipped, lag, frozen, nf, p_bf16, ema, st,
                                         group_of_range, groups);
}

int vqa_ema_update(float* ema, const float* p, long long n, float d, hipStream_t st) {
  if (!ema || !p || n < 0 || !ema_decay_ok(d)) return VQA_EARG;
  const long long nv = (((uintptr_t)ema | (uintptr_t)p) & 15) ? 0 : n / 4;
  hipLaunchKernelGGL(ema_update_kernel, dim3(blocks_of((size_t)(nv ? nv : n), 4096)), dim3(256), 0, st, ema, p, n, nv, d);
  VQA_LAUNCH_CHECK(); return VQA_OK;
}

}  // extern "C"
