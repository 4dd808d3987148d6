// Everything that reads the answer logits [B][N], for gfx950: the losses (forward + backward in one pass), the metrics, the soft answer
// scores the losses train on, and the top-k answers.  One 64-lane wave owns one row, four rows per workgroup.
//   CE                        training/train.py:120 (nn.CrossEntropyLoss and its constructor options)
//   accuracy / challenge      utils/metrics.py:55-94 VQAAccuracy, :12-19, :136-184 VQAChallengeAccuracy
//   softmax + topk            VQAModel.predict / api/inference.py:228-246
// TWO loss bodies: hard targets (cross_entropy_kernel<T, OPTS>: plain, and with class weights / ignore_index / label smoothing) and
// sparse soft targets (soft_loss_kernel<T, BCE>: softmax cross-entropy and sigmoid BCE).  What every kernel here needs is written
// once: the row maximum (row_max), the loss term / *err emission (emit_term), the rank rule of the accuracy counters (outranks,
// count_rank), arg-max -> thirds of the challenge accuracy (row_thirds, block_add_thirds) and the launch (launch_loss).  The forms of
// one body give the same bits for the same inputs because they run the same statements, not because copies agree.
#include "common.h"

__device__ __forceinline__ int lane_i(int v, int k) { return __builtin_amdgcn_readlane(v, k); }                    // k wave-uniform
__device__ __forceinline__ float lane_f(float v, int k) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), k)); }
__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return v;
}
template <typename T>
__device__ __forceinline__ float row_max(const T* __restrict__ lr, int N, int lane) {
  float m = -INFINITY;
  for (int c = lane; c < N; c += 64) m = fmaxf(m, to_f<T>(lr[c]));
  return wave_max(m);
}
// lane 0 of a row: the loss term goes to the row's slot of ws (B floats, folded in row order by a second launch: bit-reproducible)
// or, without ws, into *loss as one float atomic per row.  A bad row (a target / slot id that would read out of bounds: it raises in
// the reference) is counted in *err -- the host mirror raises from it -- and its term and gradient row are NaN.
__device__ __forceinline__ void emit_term(float term, bool bad, int row, float* part, float* loss, int* err) {
  if (part) part[row] = term;
  else if (loss) atomicAdd(loss, term);
  if (bad && err) atomicAdd(err, 1);
}
// VQAAccuracy.update without its .cpu()/.item() syncs: rank of the target = #{j : x[j] > x[t]} + #{j < t : x[j] == x[t]} (ties resolve
// to the lowest index, like argmax); top-1 correct <=> rank == 0, top-5 correct <=> rank < 5.  counters = {correct, correct_top5,
// total} (u64, +=).  A target outside [0, N) counts as wrong (the reference's comparison can never match it either).
__device__ __forceinline__ float outranks(float v, float xt, int j, int t) { return (v > xt || (v == xt && j < t)) ? 1.f : 0.f; }
__device__ __forceinline__ void count_rank(unsigned long long* counters, bool valid, float rank) {        // lane 0; rank summed over the wave
  if (valid && rank < 0.5f) atomicAdd(counters + 0, 1ull);
  if (valid && rank < 4.5f) atomicAdd(counters + 1, 1ull);
  atomicAdd(counters + 2, 1ull);
}
// The challenge accuracy (ten annotator answers per question, acc(ans) = min(1, #agreeing annotators / 3)) is counted in integer
// THIRDS: acc[0] += min(3, votes for the arg-max), acc[1] += 1 per question -- exact and independent of the order the rows arrive in.
// best: per lane, the lowest index that holds the row maximum (N: none); lane k < K holds slot k, crow = the row's counts.  Returns the
// votes for the arg-max among the row's slots, capped at 3; the same value in every lane.
__device__ __forceinline__ int row_thirds(int best, int id, const int* __restrict__ crow, int K, int lane) {
  best = wave_min_i(best);
  int votes = (lane < K && id == best) ? crow[lane] : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) votes += __shfl_xor(votes, o, 64);
  return min(3, max(0, votes));
}
// The four rows of a workgroup are added up in LDS first: one atomic pair per workgroup instead of one per row (atomics on one address
// are serialised).  Every thread of the workgroup calls this (it holds a barrier); `thirds` < 0: this wave has no row.
__device__ __forceinline__ void block_add_thirds(unsigned long long* acc, int thirds) {
  __shared__ int sh[4];
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = thirds;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0ull, n = 0ull;
#pragma unroll
    for (int w = 0; w < 4; ++w) if (sh[w] >= 0) { t += (unsigned long long)sh[w]; n += 1ull; }
    if (n) { atomicAdd(acc + 0, t); atomicAdd(acc + 1, n); }
  }
}

// ---------------------------------------------------------------------------------------------
// Hard targets: cross entropy (mean) forward+backward in one pass.  OPTS = false is the plain loss of the benchmarked step: the options
// are compile-time constants (no weights, nothing ignored, eps = 0, no counters, W = (float)B) and their branches fall out.
// OPTS = true takes nn.CrossEntropyLoss's constructor options: class weights w[N], ignore_index and label smoothing eps, reduction
// "mean".  keep[b] = target b is not ignore_index, wy[b] = keep[b] * w[t_b], W = sum_b wy[b], Sw = sum_c w[c], lp = log_softmax(x):
//   loss    += [ (1-eps) * sum_b wy[b] * (-lp[b][t_b]) + eps/N * sum_b keep[b] * sum_c w[c] * (-lp[b][c]) ] / W
//   dlogits  = [ (1-eps) * wy[b] * (p[b][c] - [c == t_b]) + eps/N * keep[b] * (Sw * p[b][c] - w[c]) ] * gscale / W
// With the options at their defaults W is (float)B, the factor (1-eps) * wy is 1.0f and the smoothing branch is not taken: the bits of
// the plain form, by the same statements.
// W and Sw are needed before the first gradient element: EVERY wave sums the B gathered weights and the N weights itself, lane c
// taking the indices c, c + 64, ... in ascending order and then the butterfly -- one fixed order, the same bits in every wave, no
// second launch and no host sync.  (Without weights W is a count of kept rows, taken in integers.)
// sum_c w[c] * lp[c] = sum_c w[c] * (x[c] - m) - log(s) * Sw rides in the pass that forms s = sum exp(x - m); x - m instead of the
// plain x keeps the cancellation against lse * Sw out of it when a row sits at +-300.  With weights or smoothing the whole row is
// evaluated in that log-softmax form, lp = (x - m) - log(s), which stays at fp32 accuracy for rows far from zero; without them
// the kernel keeps lse = m + log(s), lse - x_t and exp(x - lse) for the plain form's bits (and its accuracy there).
// A bad target (outside [0, N) and not ignore_index): see emit_term; it counts in W with weight 1 (unweighted: W = number of rows
// that are not ignored, so the default call divides by B).
// W == 0 (every row ignored, or every kept row has weight 0): the loss is NaN as in torch, dlogits is ZERO (torch: zero
// unweighted, NaN weighted -- a deliberate deviation, the step then runs on a zero gradient) and *empty += 1.
// acc = VQAAccuracy's {correct, correct_top5, total} over the kept rows (outranks / count_rank), in the same pass.
// ---------------------------------------------------------------------------------------------
struct CeOpts { const float* cw; long long ignore_index; int has_ignore; float eps; unsigned long long* acc; int* empty; };

template <typename T, bool OPTS>
__global__ __launch_bounds__(256) void cross_entropy_kernel(const T* __restrict__ logits, T* __restrict__ dlogits, const long long* __restrict__ targets,
                                                            float* loss, float* __restrict__ logits_f32, int B, int N, float gscale, int* err,
                                                            float* part, CeOpts o) {
  const float* __restrict__ cw = OPTS ? o.cw : nullptr;
  const int has_ignore = OPTS ? o.has_ignore : 0;
  const float eps = OPTS ? o.eps : 0.f;
  unsigned long long* acc = OPTS ? o.acc : nullptr;
  const int lane = threadIdx.x & 63;
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (row >= B) return;                                                 // (wave-uniform: a wave owns one row)
  float W = (float)B, Sw = (float)N;
  if (OPTS && cw) {
    float a = 0.f;
    for (int b = lane; b < B; b += 64) {
      const long long tb = targets[b];
      float w = 0.f;
      if (!(has_ignore && tb == o.ignore_index)) {
        w = 1.f;                                                        // a bad target: never read out of bounds
        if (tb >= 0 && tb < (long long)N) w = cw[tb];
      }
      a += w;
    }
    W = wave_sum(a);
    a = 0.f;
    for (int c = lane; c < N; c += 64) a += cw[c];
    Sw = wave_sum(a);
  } else if (OPTS) {
    int k = 0;
    for (int b = lane; b < B; b += 64) k += (has_ignore && targets[b] == o.ignore_index) ? 0 : 1;
#pragma unroll
    for (int q = 32; q > 0; q >>= 1) k += __shfl_xor(k, q, 64);
    W = (float)k;
  }
  const bool none = OPTS && W == 0.f;
  if (row == 0 && lane == 0 && none && o.empty) atomicAdd(o.empty, 1);
  const T* lr = logits + (size_t)row * N;
  const long long t64 = targets[row];
  if (has_ignore && t64 == o.ignore_index) {                            // ignored: no loss term, a zero gradient row, not counted
    if (lane == 0) emit_term(none ? __builtin_nanf("") : 0.f, false, row, part, loss, err);
    for (int c = lane; c < N; c += 64) {
      if (logits_f32) logits_f32[(size_t)row * N + c] = to_f<T>(lr[c]);
      if (dlogits) dlogits[(size_t)row * N + c] = from_f<T>(0.f);
    }
    return;
  }
  const bool bad = t64 < 0 || t64 >= (long long)N;
  const int t = bad ? 0 : (int)t64;
  const bool smooth = eps != 0.f;
  const bool lsm = smooth || cw;                                        // log-softmax form (see above); else the plain form's
  const float m = row_max(lr, N, lane);
  const float xt = to_f<T>(lr[t]);
  float s = 0.f, wx = 0.f, rank = 0.f;
  for (int c = lane; c < N; c += 64) {
    const float x = to_f<T>(lr[c]);
    s += expf(x - m);
    if (smooth) wx += (cw ? cw[c] : 1.f) * (x - m);
    if (acc) rank += outranks(x, xt, c, t);
  }
  s = wave_sum(s);
  if (smooth) wx = wave_sum(wx);
  if (acc) rank = wave_sum(rank);
  const float logs = logf(s);
  const float lse = m + logs;
  const float c1 = (1.f - eps) * (bad || !cw ? 1.f : cw[t]);            // (1-eps) * wy
  const float epsn = eps / (float)N;
  if (lane == 0) {
    float term = c1 * (lsm ? logs - (xt - m) : lse - xt);
    if (smooth) term += epsn * (logs * Sw - wx);
    emit_term((bad || none) ? __builtin_nanf("") : term / W, bad, row, part, loss, err);
    if (acc) count_rank(acc, !bad, rank);                               // a bad target counts as wrong
  }
  for (int c = lane; c < N; c += 64) {
    const float x = to_f<T>(lr[c]);
    if (logits_f32) logits_f32[(size_t)row * N + c] = x;
    if (dlogits) {
      const float p = lsm ? expf((x - m) - logs) : expf(x - lse);
      float g = c1 * (p - (c == t ? 1.f : 0.f));
      if (smooth) g += epsn * (Sw * p - (cw ? cw[c] : 1.f));
      g = g * gscale / W;
      dlogits[(size_t)row * N + c] = from_f<T>(bad ? __builtin_nanf("") : (none ? 0.f : g));
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Sparse soft targets (VQA v2: the soft answer scores of vqa_answer_scores): sum_k w_k * onehot(id_k) in place of the one-hot target.
// Lane k holds slot k: id -1 is an empty slot; an id < -1 or >= N is handled like a bad hard target (emit_term).
// BCE = false, softmax cross-entropy (the hard kernel's operation order; with K = 1 and weight 1 every value is the same bits):
//   loss    += (1/B) * sum_b [ W_b * lse_b - sum_k w_k * x[id_k] ],  W_b = sum_k w_k        dlogits = (W_b * p - t) * gscale / B
// BCE = true, sigmoid + binary cross-entropy (every answer is its own yes/no problem, so several annotator answers can be right at
// once and a question without an in-vocabulary answer still pushes every logit down):
//   loss    += (1/B) * sum_b sum_c [ max(x,0) + log1p(exp(-|x|)) - x*t ]      (F.binary_cross_entropy_with_logits, "sum", / B)
//   dlogits  = (sigmoid(x) - t) * gscale / B
// The row statistic (sum of exp(x - m), or the softplus sum) runs over the whole row (lane c takes c, c + 64, ... in ascending order,
// then the butterfly); the x*t part comes from the K slots in slot order.  Both BCE forms are the stable ones: exp only ever sees
// -|x|, so x = +-90 stays finite, and sigmoid(x) = {1, e} / (1 + e) with e = exp(-|x|).  A row with t == 0 everywhere is NOT a zero
// row under BCE (under cross-entropy it is): it gets sigmoid(x) * gscale / B.
// The challenge accuracy of the same rows rides along (acc: the arg-max is the lowest index that holds the row maximum the softmax
// needs anyway; BCE takes the maximum only for it).
// The store loop is one text with two trip counts: BCE runs it wave-uniform (c - lane uniform, the body masked by c < N), so the
// readlanes inside it are executed by every lane; the softmax form stops each lane at its own last column, as it always did -- the
// uniform form computes the same values there but costs it 2 us of 21 at 512 x 1000 (profiles/loss_ops_ab.txt C).
// ---------------------------------------------------------------------------------------------
template <typename T, bool BCE>
__global__ __launch_bounds__(256) void soft_loss_kernel(const T* __restrict__ logits, T* __restrict__ dlogits, const int* __restrict__ ids,
                                                        const float* __restrict__ weights, int K, float* loss, float* __restrict__ logits_f32, int B,
                                                        int N, float gscale, int* err, float* part, const int* __restrict__ counts,
                                                        unsigned long long* acc) {
  const int lane = threadIdx.x & 63;
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  int thirds = -1;
  if (row < B) {                                                         // (wave-uniform: a wave owns one row)
    const T* lr = logits + (size_t)row * N;
    const bool argmax = !BCE || acc;
    float m = -INFINITY;
    if (argmax) m = row_max(lr, N, lane);
    float s = 0.f;
    int best = N;
    for (int c = lane; c < N; c += 64) {
      const float x = to_f<T>(lr[c]);
      s += BCE ? fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))) : expf(x - m);
      if (argmax && x == m) best = min(best, c);                         // arg-max, ties -> lowest index (c ascends per lane)
    }
    s = wave_sum(s);
    const int id = lane < K ? ids[(size_t)row * K + lane] : -1;
    const bool used = id >= 0 && id < N;                                 // never read out of bounds
    const bool bad = __ballot(id < -1 || id >= N) != 0ull;
    const float w = used ? weights[(size_t)row * K + lane] : 0.f;
    const float xk = used ? to_f<T>(lr[id]) : 0.f;
    float W = 0.f, dot = 0.f;
    for (int k = 0; k < K; ++k) {                                        // slot order: W = sum_k w_k, dot = sum_k w_k * x[id_k] = sum_c x[c] * t[c]
      const float wk = lane_f(w, k);
      W += wk;
      dot += wk * lane_f(xk, k);
    }
    const float lse = m + logf(s);
    if (lane == 0) emit_term(bad ? __builtin_nanf("") : ((BCE ? s : W * lse) - dot) / (float)B, bad, row, part, loss, err);
    if (!BCE || dlogits || logits_f32) {
      for (int c = lane; (BCE ? c - lane : c) < N; c += 64) {            // BCE: a uniform trip count, masked by `in` (see above)
        const bool in = c < N;
        const float x = in ? to_f<T>(lr[c]) : 0.f;
        if (in && logits_f32) logits_f32[(size_t)row * N + c] = x;
        if (dlogits) {
          float t = 0.f;
          for (int k = 0; k < K; ++k) {                                  // duplicates add up
            const int idk = lane_i(id, k);
            const float wk = lane_f(w, k);
            t += idk == c ? wk : 0.f;
          }
          float p;
          if (BCE) {
            const float e = expf(-fabsf(x));
            p = (x >= 0.f ? 1.f : e) / (1.f + e);
          } else p = W * expf(x - lse);
          if (in) dlogits[(size_t)row * N + c] = from_f<T>(bad ? __builtin_nanf("") : (p - t) * gscale / (float)B);
        }
      }
    }
    if (acc) thirds = row_thirds(best, id, counts + (size_t)row * K, K, lane);
  }
  if (acc) block_add_thirds(acc, thirds);                                // (holds a barrier: reached by every thread, row or not)
}

// ---------------------------------------------------------------------------------------------
// The metrics alone (evaluation) and the soft answer scores.
//   vqa_accuracy_update            VQAAccuracy's counters (outranks / count_rank)
//   vqa_challenge_accuracy_update  VQAChallengeAccuracy's thirds (row_thirds / block_add_thirds)
//   vqa_answer_scores              annotator ids [B][A] -> sparse soft targets {ids, counts, weights} [B][A]
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void accuracy_kernel(const float* __restrict__ logits, const long long* __restrict__ targets,
                                                       unsigned long long* counters, int B, int N) {
  const int lane = threadIdx.x & 63;
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (row >= B) return;
  const long long t = targets[row];
  const float* x = logits + (size_t)row * N;
  float cnt = 0.f;
  const bool valid = t >= 0 && t < N;
  if (valid) {
    const float xt = x[t];
    for (int j = lane; j < N; j += 64) cnt += outranks(x[j], xt, j, (int)t);
  }
  cnt = wave_sum(cnt);
  if (lane == 0) count_rank(counters, valid, cnt);
}

__global__ __launch_bounds__(256) void challenge_accuracy_kernel(const float* __restrict__ logits, const int* __restrict__ ids, const int* __restrict__ counts,
                                                                 int K, unsigned long long* acc, int B, int N) {
  const int lane = threadIdx.x & 63;
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  int thirds = -1;
  if (row < B) {
    const float* x = logits + (size_t)row * N;
    const float m = row_max(x, N, lane);
    int best = N;
    for (int c = lane; c < N; c += 64) if (x[c] == m) best = min(best, c);
    thirds = row_thirds(best, lane < K ? ids[(size_t)row * K + lane] : -1, counts + (size_t)row * K, K, lane);
  }
  block_add_thirds(acc, thirds);
}

__global__ __launch_bounds__(256) void answer_scores_kernel(const long long* __restrict__ answers, int* __restrict__ ids, float* __restrict__ weights,
                                                            int* __restrict__ counts, int B, int A, int N, int mode, int* err) {
  const int lane = threadIdx.x & 63;
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (row >= B) return;
  const long long a = lane < A ? answers[(size_t)row * A + lane] : -1ll;
  const bool valid = a >= 0 && a < (long long)N;                       // -1: the annotator's answer is not in the vocabulary
  const bool rowbad = __ballot(a < -1ll || a >= (long long)N) != 0ull;
  const int ai = valid ? (int)a : -1;                                  // (a valid id is below N: it fits)
  int cnt = 0, earlier = 0;
  for (int j = 0; j < A; ++j) {
    const int aj = lane_i(ai, j);                                      // read by EVERY lane: never under a divergent condition
    const int same = (valid && aj == ai) ? 1 : 0;
    cnt += same;
    earlier += j < lane ? same : 0;
  }
  const bool first = valid && earlier == 0;
  const unsigned long long firsts = __ballot(first);                  // distinct ids, in order of first occurrence
  const int slot = __popcll(firsts & ((1ull << lane) - 1ull)), nslots = __popcll(firsts);
  float w = first ? fminf(1.f, (float)cnt / 3.f) : 0.f;
  if (mode == 1) {                                                     // rows sum to one: the sum is taken in slot order
    float s = 0.f;
    for (unsigned long long m = firsts; m; m &= m - 1ull) s += __shfl(w, __ffsll((long long)m) - 1, 64);
    if (first && s > 0.f) w = w / s;
  }
  const size_t o = (size_t)row * A;
  if (rowbad) {                                                        // slot 0 carries the id N: the loss kernel rejects the row
    if (lane < A) { ids[o + lane] = lane == 0 ? N : -1; weights[o + lane] = 0.f; counts[o + lane] = 0; }
    if (lane == 0 && err) atomicAdd(err, 1);
    return;
  }
  if (first) { ids[o + slot] = (int)a; weights[o + slot] = w; counts[o + slot] = cnt; }
  if (lane >= nslots && lane < A) { ids[o + lane] = -1; weights[o + lane] = 0.f; counts[o + lane] = 0; }
}

// ---------------------------------------------------------------------------------------------
// Top-k answers with their softmax probabilities (softmax + topk), one launch.  y[j] = logits[j] where allowed (or without a mask),
// else -inf.  Index a ranks before b when y[a] > y[b], or y[a] == y[b] and a < b (the lowest-index tie rule of outranks); NaN ranks
// above every number, NaNs among themselves by index: torch.sort(y, descending=True, stable=True).  The order is decided on y alone,
// through an order-preserving 32-bit key (NaN -> all ones, -0 == +0) joined with the reversed index into one 64-bit word, so a pick is
// an integer maximum.  probs = exp(scale * y - m) / sum_j exp(scale * y[j] - m), m = max_j scale * y[j] (NaNs skipped by the max, so a
// row that holds a NaN, or nothing but -inf, gives NaN for every probability as torch.softmax does).  K rounds, each the best word
// strictly below the previous pick: no per-row state, no atomics, no LDS.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t topk_key(float y) {
  if (y != y) return 0xffffffffu;
  uint32_t b = __float_as_uint(y);
  if (b == 0x80000000u) b = 0u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float topk_val(uint32_t k) {          // inverse of topk_key (the all-ones key gives a NaN)
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ unsigned long long topk_word(uint32_t key, int j) {
  return ((unsigned long long)key << 32) | (unsigned long long)(0x7fffffffu - (uint32_t)j);
}
__device__ __forceinline__ float topk_arg(float scale, float y, float m) {      // scale * y - m with both roundings (never one fma)
#pragma clang fp contract(off)
  const float s = scale * y;
  return s - m;
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t hi = __shfl_xor((uint32_t)(v >> 32), o, 64), lo = __shfl_xor((uint32_t)v, o, 64);
    const unsigned long long w = ((unsigned long long)hi << 32) | lo;
    v = w > v ? w : v;
  }
  return v;
}

// The row is read again in each of the K + 2 passes (L2-resident: 4 KB at N = 1000).
template <typename T>
__global__ __launch_bounds__(256) void softmax_topk_kernel(const T* __restrict__ logits, long long ld, const unsigned char* __restrict__ allowed,
                                                           long long allowed_ld, float scale, long long* __restrict__ idx,
                                                           float* __restrict__ probs, float* __restrict__ logits_f, int B, int N, int K) {
  const int lane = threadIdx.x & 63;
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (row >= B) return;
  const T* x = logits + (size_t)row * ld;
  const unsigned char* al = allowed ? allowed + (size_t)row * allowed_ld : nullptr;
  float* xf = logits_f ? logits_f + (size_t)row * N : nullptr;
  auto y_at = [&](int j) -> float {
    const float v = to_f<T>(x[j]);
    return (al && !al[j]) ? -INFINITY : v;
  };
  // pass 1: raw fp32 copy, row maximum of scale * y
  float m = -INFINITY;
  for (int j = lane; j < N; j += 64) {
    if (xf) xf[j] = to_f<T>(x[j]);
    m = fmaxf(m, scale * y_at(j));
  }
  m = wave_max(m);
  // pass 2: denominator, per lane in index order, then the butterfly (a fixed order: bit-reproducible)
  float sum = 0.f;
  for (int j = lane; j < N; j += 64) sum += expf(topk_arg(scale, y_at(j), m));
  sum = wave_sum(sum);
  // K rounds of selection; lane r keeps pick r
  unsigned long long prev = ~0ull, mine = 0ull;
  for (int r = 0; r < K; ++r) {
    unsigned long long best = 0ull;
    for (int j = lane; j < N; j += 64) {
      const unsigned long long c = topk_word(topk_key(y_at(j)), j);
      if (c < prev && c > best) best = c;
    }
    best = wave_max_u64(best);
    prev = best;
    if (lane == r) mine = best;
  }
  if (lane < K) {
    const float y = topk_val((uint32_t)(mine >> 32));
    idx[(size_t)row * K + lane] = (long long)(0x7fffffffu - (uint32_t)mine);
    probs[(size_t)row * K + lane] = expf(topk_arg(scale, y, m)) / sum;
  }
}

// ---------------------------------------------------------------------------------------------
// The launch of every loss: one wave per row, fp32 or bf16 logits (dtype 0 / 1), and with ws (B floats) the fold of the row terms in
// row order right behind it (fold_rows_kernel, token_ops.hip); without ws the kernel adds one float atomic per row.  *loss is
// accumulated into (+=): zero it first.  `Same` keeps the kernel's signature, not the call, in charge of the argument types.
// ---------------------------------------------------------------------------------------------
static inline dim3 row_grid(int B) { return dim3((B + 3) / 4); }
template <typename X> struct Same { using type = X; };
template <typename T, typename... A> using LossKernel = void (*)(const T*, T*, A...);

template <typename... A>
static int launch_loss(LossKernel<float, A...> kf, LossKernel<bf16_t, A...> kb, int dtype, const void* logits, void* dlogits, int B, float* loss,
                       float* ws, hipStream_t st, typename Same<A>::type... a) {
  if (dtype) hipLaunchKernelGGL(kb, row_grid(B), dim3(256), 0, st, (const bf16_t*)logits, (bf16_t*)dlogits, a...);
  else hipLaunchKernelGGL(kf, row_grid(B), dim3(256), 0, st, (const float*)logits, (float*)dlogits, a...);
  if (ws && loss) vqa_launch_fold(ws, B, 1, 1, loss, 1, nullptr, st);     // B "rows" of one column
  VQA_LAUNCH_CHECK(); return VQA_OK;
}

extern "C" {

// ws (B floats or nullptr), *loss: see launch_loss.  Nothing is launched on an argument error.
int vqa_cross_entropy(int dtype, const void* logits, const long long* targets, float* loss, void* dlogits, float* logits_f32, int B, int N,
                      float gscale, int* err, float* ws, hipStream_t st) {
  if (!logits || !targets || B <= 0 || N <= 0) return VQA_EARG;
  return launch_loss(cross_entropy_kernel<float, false>, cross_entropy_kernel<bf16_t, false>, dtype, logits, dlogits, B, loss, ws, st,
                     targets, loss, logits_f32, B, N, gscale, err, ws, CeOpts{});
}
// vqa_cross_entropy's arguments, then the options; class_weight nullptr = all ones, has_ignore 0 = no target is ignored, acc / empty
// optional.
int vqa_cross_entropy_opts(int dtype, const void* logits, const long long* targets, float* loss, void* dlogits, float* logits_f32,
                           int B, int N, float gscale, int* err, float* ws, const float* class_weight, long long ignore_index,
                           int has_ignore, float label_smoothing, unsigned long long* acc, int* empty, hipStream_t st) {
  if (!logits || !targets || B <= 0 || N <= 0 || (dtype != 0 && dtype != 1)) return VQA_EARG;
  if (!(label_smoothing >= 0.f && label_smoothing <= 1.f) || !(fabsf(gscale) <= 3.402823466e38f)) return VQA_EARG;   // (NaN fails both)
  return launch_loss(cross_entropy_kernel<float, true>, cross_entropy_kernel<bf16_t, true>, dtype, logits, dlogits, B, loss, ws, st,
                     targets, loss, logits_f32, B, N, gscale, err, ws, CeOpts{class_weight, ignore_index, has_ignore, label_smoothing, acc, empty});
}
// vqa_cross_entropy with sparse soft targets (ids, weights [B][K]); counts + acc: the challenge accuracy of the same rows
int vqa_cross_entropy_soft(int dtype, const void* logits, const int* ids, const float* weights, int K, float* loss, void* dlogits,
                           float* logits_f32, int B, int N, float gscale, int* err, float* ws, const int* counts,
                           unsigned long long* acc, hipStream_t st) {
  if (!logits || !ids || !weights || K <= 0 || K > 64 || B <= 0 || N <= 0 || (acc && !counts)) return VQA_EARG;
  return launch_loss(soft_loss_kernel<float, false>, soft_loss_kernel<bf16_t, false>, dtype, logits, dlogits, B, loss, ws, st,
                     ids, weights, K, loss, logits_f32, B, N, gscale, err, ws, counts, acc);
}
// vqa_cross_entropy_soft's arguments
int vqa_bce_soft(int dtype, const void* logits, const int* ids, const float* weights, int K, float* loss, void* dlogits,
                 float* logits_f32, int B, int N, float gscale, int* err, float* ws, const int* counts, unsigned long long* acc,
                 hipStream_t st) {
  if (!logits || !ids || !weights || K < 1 || K > 64 || B < 1 || N < 1 || (acc && !counts) || (dtype != 0 && dtype != 1)) return VQA_EARG;
  if (!(fabsf(gscale) <= 3.402823466e38f)) return VQA_EARG;              // (NaN fails the comparison too)
  return launch_loss(soft_loss_kernel<float, true>, soft_loss_kernel<bf16_t, true>, dtype, logits, dlogits, B, loss, ws, st,
                     ids, weights, K, loss, logits_f32, B, N, gscale, err, ws, counts, acc);
}

int vqa_accuracy_update(const float* logits, const long long* targets, unsigned long long* counters, int B, int N, hipStream_t st) {
  if (!logits || !targets || !counters || B <= 0 || N <= 0) return VQA_EARG;
  hipLaunchKernelGGL(accuracy_kernel, row_grid(B), dim3(256), 0, st, logits, targets, counters, B, N);
  VQA_LAUNCH_CHECK(); return VQA_OK;
}
int vqa_challenge_accuracy_update(const float* logits, const int* ids, const int* counts, int K, unsigned long long* acc, int B, int N,
                                  hipStream_t st) {
  if (!logits || !ids || !counts || !acc || K <= 0 || K > 64 || B <= 0 || N <= 0) return VQA_EARG;
  hipLaunchKernelGGL(challenge_accuracy_kernel, row_grid(B), dim3(256), 0, st, logits, ids, counts, K, acc, B, N);
  VQA_LAUNCH_CHECK(); return VQA_OK;
}
int vqa_answer_scores(const long long* answers, int* ids, float* weights, int* counts, int B, int A, int N, int mode, int* err,
                      hipStream_t st) {
  if (!answers || !ids || !weights || !counts || B <= 0 || A <= 0 || A > 64 || N <= 0 || (mode != 0 && mode != 1)) return VQA_EARG;
  hipLaunchKernelGGL(answer_scores_kernel, row_grid(B), dim3(256), 0, st, answers, ids, weights, counts, B, A, N, mode, err);
  VQA_LAUNCH_CHECK(); return VQA_OK;
}
int vqa_softmax_topk(int dtype, const void* logits, long long ld, const unsigned char* allowed, long long allowed_ld, float scale,
                     long long* idx, float* probs, float* logits_f, int B, int N, int K, hipStream_t st) {
  if (!logits || !idx || !probs || B < 1 || N < 1 || K < 1 || K > 64 || K > N || ld < N || (allowed_ld != 0 && allowed_ld < N)
      || !(scale > 0.f) || !(scale <= 3.402823466e38f) || (dtype != 0 && dtype != 1)) return VQA_EARG;
  if (dtype) hipLaunchKernelGGL(softmax_topk_kernel<bf16_t>, row_grid(B), dim3(256), 0, st, (const bf16_t*)logits, ld, allowed, allowed_ld, scale, idx,
                                probs, logits_f, B, N, K);
  else hipLaunchKernelGGL(softmax_topk_kernel<float>, row_grid(B), dim3(256), 0, st, (const float*)logits, ld, allowed, allowed_ld, scale, idx, probs,
                          logits_f, B, N, K);
  VQA_LAUNCH_CHECK(); return VQA_OK;
}

}  // extern "C"
