// Explaining an answer on the device, for gfx950: the four launches around the backward that stops at the image features
// (engine.explain_route; VQAModel.explain / Explanation.render).
//   vqa_class_seed       the class to explain (given, or the row's arg-max) and the one-hot seed of its backward
//   vqa_gradcam          Grad-CAM of the NHWC features: channel weights = spatial mean of the gradient, ReLU of the weighted sum
//   vqa_attention_map    mean of the cross-attention probabilities over layers, heads and the question's real tokens
//   vqa_heatmap_render   bilinear upsample (F.interpolate, align_corners=False) -> colour table -> blend over the image, uint8 out
// Every sum is fp32 in a fixed order (per-thread index order, then LDS partials in index order, then the wave butterfly): no float
// atomics, the same bits on every run.  Shapes a kernel does not take are refused with VQA_EARG before any launch.
#include "common.h"

// ---------------------------------------------------------------------------------------------
// vqa_class_seed: one wave per row, four rows per workgroup.  The arg-max uses vqa_softmax_topk's order (loss_ops.hip): an
// order-preserving 32-bit key of the value (NaN -> all ones: it ranks first; -0 == +0) joined with the reversed index, so the
// pick is an integer maximum and ties go to the lower index.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long seed_word(float y, int j) {
  uint32_t key = 0xffffffffu;
  if (y == y) {
    uint32_t b = __float_as_uint(y);
    if (b == 0x80000000u) b = 0u;
    key = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  }
  return ((unsigned long long)key << 32) | (unsigned long long)(0x7fffffffu - (uint32_t)j);
}
template <typename T>
__global__ __launch_bounds__(256) void class_seed_kernel(const T* __restrict__ logits, long long ld, const long long* __restrict__ ids,
                                                         long long* __restrict__ chosen, T* __restrict__ dlogits, int B, int N) {
  const int lane = threadIdx.x & 63;
  const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (row >= B) return;
  long long c;
  if (ids) c = ids[row];
  else {
    const T* x = logits + (size_t)row * ld;
    unsigned long long best = 0ull;
    for (int j = lane; j < N; j += 64) {
      const unsigned long long w = seed_word(to_f<T>(x[j]), j);
      best = w > best ? w : best;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const uint32_t hi = __shfl_xor((uint32_t)(best >> 32), o, 64), lo = __shfl_xor((uint32_t)best, o, 64);
      const unsigned long long w = ((unsigned long long)hi << 32) | lo;
      best = w > best ? w : best;
    }
    c = (long long)(0x7fffffffu - (uint32_t)best);
  }
  if (lane == 0) chosen[row] = c;
  T* d = dlogits + (size_t)row * N;
  for (int j = lane; j < N; j += 64) d[j] = from_f<T>((long long)j == c ? 1.f : 0.f);
}

// row maximum of values held one per thread-visit, over the 256 threads of a workgroup (NaNs are skipped, as fmaxf does)
__device__ __forceinline__ float block_max_256(float v, float* sh4) {
  v = wave_max(v);
  __syncthreads();                                   // (sh4 may still be read from an earlier use)
  if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(sh4[0], sh4[1]), fmaxf(sh4[2], sh4[3]));
}

// ---------------------------------------------------------------------------------------------
// vqa_gradcam: one workgroup per image.  Phase 1 reads dfeat[b] once: thread (r, g) sums the 16-byte channel group g over the
// positions p = r, r + R, ... (R = 256 / groups row lanes), the R partial rows are added in index order and divided by P.  Phase 2
// reads feat[b] once: a wave per position, 16 bytes per lane and 64-lane step, the butterfly, ReLU.  Normalisation: the
// workgroup's maximum, then every lane 0 divides the values it wrote itself.
// ---------------------------------------------------------------------------------------------
#define GRADCAM_MAX_C 1024
template <typename T>
__global__ __launch_bounds__(256) void gradcam_kernel(const T* __restrict__ feat, const T* __restrict__ dfeat, float* __restrict__ cam,
                                                      int P, int C, int normalize) {
  constexpr int VEC = Vec16<T>::N;
  __shared__ float part[256 * 8];                    // [R][C] partial channel sums, R * C <= 256 * VEC
  __shared__ float alpha[GRADCAM_MAX_C];
  __shared__ float sh4[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int groups = C / VEC, R = 256 / groups;
  const T* df = dfeat + (size_t)b * P * C;
  const T* ft = feat + (size_t)b * P * C;
  if (tid < groups * R) {
    const int g = tid % groups, r = tid / groups;
    float acc[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[j] = 0.f;
    for (int p = r; p < P; p += R) {
      const Vec16<T> v = ldg16(df + (size_t)p * C + g * VEC);
#pragma unroll
      for (int j = 0; j < VEC; ++j) acc[j] += v.get(j);
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) part[r * C + g * VEC + j] = acc[j];
  }
  __syncthreads();
  for (int c = tid; c < C; c += 256) {
    float s = 0.f;
    for (int r = 0; r < R; ++r) s += part[r * C + c];
    alpha[c] = s / (float)P;
  }
  __syncthreads();
  float* out = cam + (size_t)b * P;
  float mx = 0.f;
  for (int p = wave; p < P; p += 4) {
    float s = 0.f;
    for (int c0 = lane * VEC; c0 < C; c0 += 64 * VEC) {
      const Vec16<T> v = ldg16(ft + (size_t)p * C + c0);
#pragma unroll
      for (int j = 0; j < VEC; ++j) s += alpha[c0 + j] * v.get(j);
    }
    s = wave_sum(s);
    s = s > 0.f ? s : (s == s ? 0.f : s);            // ReLU; a NaN stays a NaN
    mx = fmaxf(mx, s);
    if (lane == 0) out[p] = s;
  }
  if (!normalize) return;
  mx = block_max_256(mx, sh4);
  if (lane == 0 && mx > 0.f) {                       // (a row whose maximum is 0 stays as it is: all zero)
    for (int p = wave; p < P; p += 4) out[p] = __fdiv_rn(out[p], mx);
  }
}

// ---------------------------------------------------------------------------------------------
// vqa_attention_map: one workgroup per question.  For fixed (layer, head) the [L][P] probabilities are contiguous: thread i owns
// the flat elements i, i + 256, ... and adds them over (layer, head) in index order into LDS (rows of padding tokens are not
// read); then thread p adds the L rows of column p in token order and divides by ncl * H * n_b (0 / 0 = NaN for a question
// without a real token).
// ---------------------------------------------------------------------------------------------
#define ATTMAP_MAX_LP 8192
__global__ __launch_bounds__(256) void attention_map_kernel(const float* __restrict__ caw, const float* __restrict__ mask,
                                                            float* __restrict__ out, int ncl, int B, int H, int L, int P, int normalize) {
  __shared__ float acc[ATTMAP_MAX_LP];
  __shared__ float sh4[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int LP = L * P;
  const float* mrow = mask ? mask + (size_t)b * L : nullptr;
  float nb = 0.f;
  for (int t = 0; t < L; ++t) nb += (!mrow || mrow[t] != 0.f) ? 1.f : 0.f;
  for (int i = tid; i < LP; i += 256) {
    const int t = i / P;
    float s = 0.f;
    if (!mrow || mrow[t] != 0.f) {
      for (int l = 0; l < ncl; ++l)
        for (int h = 0; h < H; ++h) s += caw[(((size_t)l * B + b) * H + h) * LP + i];
    }
    acc[i] = s;
  }
  __syncthreads();
  const float den = (float)(ncl * H) * nb;
  float* orow = out + (size_t)b * P;
  float mx = 0.f;
  for (int p = tid; p < P; p += 256) {
    float s = 0.f;
    for (int t = 0; t < L; ++t) s += acc[t * P + p];
    s = __fdiv_rn(s, den);
    mx = fmaxf(mx, s);
    orow[p] = s;
  }
  if (!normalize) return;
  mx = block_max_256(mx, sh4);
  if (mx > 0.f) {
    for (int p = tid; p < P; p += 256) orow[p] = __fdiv_rn(orow[p], mx);
  }
}

// ---------------------------------------------------------------------------------------------
// vqa_heatmap_render: one thread per four output pixels of a row (12 bytes: three dword loads of the base, three dword stores when
// W % 4 == 0; single bytes otherwise).  The colour table sits in LDS.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void bilinear_src(int dst, float scale, int n, int& i0, int& i1, float& w1) {
  float s = scale * ((float)dst + 0.5f) - 0.5f;      // F.interpolate, align_corners=False (area_pixel_compute_source_index)
  if (s < 0.f) s = 0.f;
  i0 = (int)s;
  if (i0 > n - 1) i0 = n - 1;
  i1 = i0 + (i0 < n - 1 ? 1 : 0);
  w1 = s - (float)i0;
}
template <bool VEC4>
__global__ __launch_bounds__(256) void heatmap_render_kernel(const float* __restrict__ map, const uint8_t* __restrict__ base,
                                                             const uint8_t* __restrict__ lut, uint8_t* __restrict__ out, int B, int Hm,
                                                             int Wm, int H, int W, float alpha, float sy, float sx, long long quads) {
  __shared__ uint8_t tab[768];
  for (int i = threadIdx.x; i < 768; i += 256) tab[i] = lut[i];
  __syncthreads();
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
  if (q >= quads) return;
  const int qw = (W + 3) / 4;
  const int xq = (int)(q % qw);
  const long long by = q / qw;
  const int y = (int)(by % H), b = (int)(by / H);
  const float* m = map + (size_t)b * Hm * Wm;
  int y0, y1; float wy;
  bilinear_src(y, sy, Hm, y0, y1, wy);
  const size_t o = (((size_t)b * H + y) * W + (size_t)xq * 4) * 3;
  const int npx = (W - xq * 4) < 4 ? (W - xq * 4) : 4;
  uint8_t px[12];
  if (base) {
    if (VEC4) {
      const uint32_t* bp = reinterpret_cast<const uint32_t*>(base + o);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const uint32_t w = bp[k];
        px[4 * k] = (uint8_t)w; px[4 * k + 1] = (uint8_t)(w >> 8); px[4 * k + 2] = (uint8_t)(w >> 16); px[4 * k + 3] = (uint8_t)(w >> 24);
      }
    } else {
      for (int k = 0; k < 12; ++k) px[k] = k < npx * 3 ? base[o + k] : (uint8_t)0;
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (k >= npx) break;
    int x0, x1; float wx;
    bilinear_src(xq * 4 + k, sx, Wm, x0, x1, wx);
    const float top = (1.f - wx) * m[y0 * Wm + x0] + wx * m[y0 * Wm + x1];
    const float bot = (1.f - wx) * m[y1 * Wm + x0] + wx * m[y1 * Wm + x1];
    const float t = (1.f - wy) * top + wy * bot;
    const float u = t * 255.f + 0.5f;
    const int idx = u >= 0.f ? (u >= 256.f ? 255 : (int)floorf(u)) : 0;          // (a NaN fails the first comparison: entry 0)
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float c = (float)tab[idx * 3 + ch];
      if (base) {
        float v = floorf(alpha * c + (1.f - alpha) * (float)px[3 * k + ch] + 0.5f);
        v = v < 0.f ? 0.f : (v > 255.f ? 255.f : v);
        px[3 * k + ch] = (uint8_t)v;
      } else px[3 * k + ch] = tab[idx * 3 + ch];
    }
  }
  if (VEC4) {
    uint32_t* op = reinterpret_cast<uint32_t*>(out + o);
#pragma unroll
    for (int k = 0; k < 3; ++k)
      op[k] = (uint32_t)px[4 * k] | ((uint32_t)px[4 * k + 1] << 8) | ((uint32_t)px[4 * k + 2] << 16) | ((uint32_t)px[4 * k + 3] << 24);
  } else {
    for (int k = 0; k < npx * 3; ++k) out[o + k] = px[k];
  }
}

extern "C" {

int vqa_class_seed(int dtype, const void* logits, long long ld, const long long* ids, long long* chosen, void* dlogits, int B, int N,
                   hipStream_t st) {
  if (!logits || !chosen || !dlogits || B < 1 || N < 1 || ld < N || (dtype != 0 && dtype != 1)) return VQA_EARG;
  const dim3 grid((B + 3) / 4);
  DT(hipLaunchKernelGGL(class_seed_kernel<float>, grid, dim3(256), 0, st, (const float*)logits, ld, ids, chosen, (float*)dlogits, B, N),
     hipLaunchKernelGGL(class_seed_kernel<bf16_t>, grid, dim3(256), 0, st, (const bf16_t*)logits, ld, ids, chosen, (bf16_t*)dlogits, B, N));
  VQA_LAUNCH_CHECK(); return VQA_OK;
}

int vqa_gradcam(int dtype, const void* feat, const void* dfeat, float* cam, int B, int P, int C, int normalize, hipStream_t st) {
  if (!feat || !dfeat || !cam || B < 1 || P < 1 || C < 8 || C % 8 || C > GRADCAM_MAX_C || (dtype != 0 && dtype != 1)) return VQA_EARG;
  if ((reinterpret_cast<uintptr_t>(feat) | reinterpret_cast<uintptr_t>(dfeat)) & 15) return VQA_EARG;      // 16-byte loads
  DT(hipLaunchKernelGGL(gradcam_kernel<float>, dim3(B), dim3(256), 0, st, (const float*)feat, (const float*)dfeat, cam, P, C, normalize),
     hipLaunchKernelGGL(gradcam_kernel<bf16_t>, dim3(B), dim3(256), 0, st, (const bf16_t*)feat, (const bf16_t*)dfeat, cam, P, C, normalize));
  VQA_LAUNCH_CHECK(); return VQA_OK;
}

int vqa_attention_map(const float* caw, const float* mask, float* out, int ncl, int B, int H, int L, int P, int normalize, hipStream_t st) {
  if (!caw || !out || ncl < 1 || B < 1 || H < 1 || L < 1 || P < 1 || (long long)L * P > ATTMAP_MAX_LP) return VQA_EARG;
  hipLaunchKernelGGL(attention_map_kernel, dim3(B), dim3(256), 0, st, caw, mask, out, ncl, B, H, L, P, normalize);
  VQA_LAUNCH_CHECK(); return VQA_OK;
}

int vqa_heatmap_render(const float* map, const uint8_t* base, const uint8_t* lut, uint8_t* out, int B, int Hm, int Wm, int H, int W,
                       float alpha, hipStream_t st) {
  if (!map || !lut || !out || B < 1 || Hm < 1 || Wm < 1 || H < 1 || W < 1 || !(alpha >= 0.f && alpha <= 1.f)) return VQA_EARG;
  const long long quads = (long long)B * H * ((W + 3) / 4);
  const long long blocks = (quads + 255) / 256;
  if (blocks > 0x7fffffffll) return VQA_EARG;
  const float sy = (float)Hm / (float)H, sx = (float)Wm / (float)W;
  const bool vec = W % 4 == 0 && !((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(base)) & 3);
  if (vec) hipLaunchKernelGGL(heatmap_render_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, map, base, lut, out, B, Hm, Wm, H, W, alpha, sy, sx, quads);
  else hipLaunchKernelGGL(heatmap_render_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, map, base, lut, out, B, Hm, Wm, H, W, alpha, sy, sx, quads);
  VQA_LAUNCH_CHECK(); return VQA_OK;
}

}  // extern "C"
