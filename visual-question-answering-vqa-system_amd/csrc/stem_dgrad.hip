// Data gradient of the stem convolution 7x7 / stride 2 / pad 3 (3 -> 64 channels): the gradient with respect to the input image.
//
//   dimg[b][c][ih][iw] = sum_{oh,ow,k} dy[b][oh][ow][k] * W[k][r][s][c],   r = ih + 3 - 2 oh,  s = iw + 3 - 2 ow  (both in 0..6)
//
// Implicit GEMM over 2x2 image quads: the quad (2i+ph, 2j+pw) only sees the 4x4 window of dy pixels oh = i-1+u, ow = j-1+v
// (u, v in 0..3) through the taps r = ph+5-2u, s = pw+5-2v (zero outside 0..6).  So M = B*Ho*Wo quads, K = 16 pixels x 64
// channels = 1024 (k = (u*4+v)*64 + channel), N = 4 phases x 3 channels = 12, padded to 16 (n = c*4 + ph*2 + pw).  Every image
// element is written exactly once: no atomics, bit-reproducible.
//
// One workgroup = (image, band of quad rows, strip of quad columns).  It walks down its band keeping the four dy rows of the current
// quad row in an LDS ring: per quad row ONE new dy row is staged (a band re-stages its 3-row halo once).  The fused entry rebuilds
// each staged dy row from the raw conv output y, the pooled gradient + argmax (stem_route_pair_buf) and the BatchNorm backward
// coefficients with the expression vqa_stem_bwd_apply uses; the generic entries copy it from a materialised dy.  Both then run the
// same MFMA loop in the same K order.  They are not always bit-equal: a rebuilt dy element can round to the neighbouring bf16 value
// of the one vqa_stem_bwd_apply stores (measured on MI355X; the tests bound the difference by one bf16 rounding of dy).
//   bf16: v_mfma_f32_16x16x32_bf16, the packed [16][1024] weight operand (32 KB) lives in registers (32 fragments per lane).
//   fp32: v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation), the packed operand (64 KB) lives in LDS.
// The quad-row results go through LDS and leave as coalesced rows of the NCHW fp32 image; rows / columns past H-1 / W-1 are masked.
#include "common.h"
#include <type_traits>
#include "stem_route.h"

namespace {
// element-wise packed operand layout: [ko][g][n][e], k = ko*CH + g*(CH/4) + e, CH = 32 (bf16) or 16 (fp32): a lane (g, n) of an
// MFMA reads its whole fragment of K chunk ko as one contiguous 16-byte vector
template <typename T> struct DG;
template <> struct DG<bf16_t> { static constexpr int CH = 32, LDP = 72, MAXSW = 128; };   // LDS pixel stride 144 B: b128 reads conflict-free
template <> struct DG<float> { static constexpr int CH = 16, LDP = 68, MAXSW = 64; };     // 272 B
constexpr int KTOT = 1024;

// sizes of one launch: SW quad columns per strip, QB quad rows per band
struct DgGeom { int Ho, Wo, SW, nstrip, QB, nband; };

template <typename T>
DgGeom dg_geom(int B, int H, int W) {
  DgGeom g;
  g.Ho = (H + 6 - 7) / 2 + 1; g.Wo = (W + 6 - 7) / 2 + 1;
  g.nstrip = (g.Wo + DG<T>::MAXSW - 1) / DG<T>::MAXSW;
  g.SW = ((g.Wo + g.nstrip - 1) / g.nstrip + 15) / 16 * 16;
  // about 2048 workgroups: long bands (few halo rows re-staged) at large B, short ones at small B
  const long long per = (long long)B * g.nstrip;
  int bands = (int)((2048 + per - 1) / per);
  bands = bands < 1 ? 1 : (bands > g.Ho ? g.Ho : bands);
  g.QB = (g.Ho + bands - 1) / bands;
  if (g.QB < 4) g.QB = g.Ho < 4 ? g.Ho : 4;
  g.nband = (g.Ho + g.QB - 1) / g.QB;
  return g;
}

template <typename T>
size_t dg_shm(int SW) {
  size_t s = (size_t)4 * (SW + 4) * DG<T>::LDP * sizeof(T) + (size_t)12 * SW * 4;
  if (std::is_same<T, float>::value) s += (size_t)16 * KTOT * 4;
  return s;
}
}  // namespace

// wpk (packed operand, [ko][g][n][e]) <- w [64][7][7][3] fp32 (KRSC master)
template <typename T>
__global__ void stem_dgrad_pack_kernel(const float* __restrict__ w, T* __restrict__ wpk) {
  constexpr int CH = DG<T>::CH, E = CH / 4;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= 16 * KTOT) return;
  const int e = idx % E, n = (idx / E) % 16, g = (idx / (E * 16)) % 4, ko = idx / (E * 64);
  const int k = ko * CH + g * E + e, uv = k >> 6, kc = k & 63, u = uv >> 2, v = uv & 3;
  float val = 0.f;
  if (n < 12) {
    const int c = n >> 2, ph = (n >> 1) & 1, pw = n & 1, r = ph + 5 - 2 * u, s = pw + 5 - 2 * v;
    if (r >= 0 && r <= 6 && s >= 0 && s <= 6) val = w[((kc * 7 + r) * 7 + s) * 3 + c];
  }
  wpk[idx] = from_f<T>(val);
}

// FUSED (bf16 only): src = y (raw conv output [B][Ho][Wo][64]) and dy is rebuilt from y, dpool, idx, coef, bc; else src = dy.
template <typename T, bool FUSED>
__global__ __launch_bounds__(256, 2) void stem_dgrad_kernel(const T* __restrict__ src, const bf16_t* __restrict__ dpool,
                                                         const uint8_t* __restrict__ idx, const float* __restrict__ coef,
                                                         const float* __restrict__ bc, const T* __restrict__ wpk, float* __restrict__ dimg,
                                                         int B, int H, int W, int Ho, int Wo, int Hp, int Wp, int SW, int nstrip, int QB,
                                                         int nband) {
  constexpr bool BF = std::is_same<T, bf16_t>::value;
  constexpr int CH = DG<T>::CH, LDP = DG<T>::LDP, VEC = Vec16<T>::N;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int PX = SW + 4;                                          // staged pixels: ow = j0-2 .. j0+SW+1
  T* ring = reinterpret_cast<T*>(smem);                           // [4][PX][LDP]: dy row oh in slot (oh + 1) & 3
  float* ost = reinterpret_cast<float*>(ring + 4 * PX * LDP);     // [3][2][2*SW]: one quad row of the image gradient
  float* bl = ost + 12 * SW;                                      // fp32: packed operand [16*1024]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
  int blk = blockIdx.x;
  const int strip = blk % nstrip; blk /= nstrip;
  const int band = blk % nband;
  const int b = blk / nband;
  const int j0 = strip * SW, i0 = band * QB, i1 = min(Ho, i0 + QB);

  // ---- weight operand
  bf16x8 bw[BF ? KTOT / CH : 1];
  if constexpr (BF) {
#pragma unroll
    for (int t = 0; t < KTOT / CH; ++t)
      bw[t] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(wpk + ((t * 4 + g) * 16 + li) * 8));
  } else {
    for (int i = tid; i < 16 * KTOT / 4; i += 256)
      reinterpret_cast<u32x4*>(bl)[i] = reinterpret_cast<const u32x4*>(wpk)[i];
  }

  // ---- staging of one dy row into its ring slot (zeros outside the conv output)
  float f_sc[8], f_sh[8], f_a[8], f_b[8], f_c[8];
  const __amdgpu_buffer_rsrc_t rsP = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(dpool), 0, FUSED ? B * Hp * Wp * 64 * 2 : 0, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsI = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(idx), 0, FUSED ? B * Hp * Wp * 64 : 0, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsY = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(src), 0, FUSED ? B * Ho * Wo * 64 * 2 : 0, 0x00020000);
  if constexpr (FUSED) {
    const int c0f = (tid & 7) * 8;                                // 256 % 8 == 0: this thread always stages channel vector tid & 7
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      f_sc[j] = coef[c0f + j]; f_sh[j] = coef[64 + c0f + j];
      f_a[j] = bc[c0f + j]; f_b[j] = bc[64 + c0f + j]; f_c[j] = bc[128 + c0f + j];
    }
  }
  auto stage = [&](int oh) {
    T* dst = ring + ((oh + 1) & 3) * PX * LDP;
    const bool rok = oh >= 0 && oh < Ho;
    if constexpr (FUSED) {
      // items = (pixel pair (ow, ow+1), ow = j0-2+2p even, channel vector): the pair shares its pooling windows
      auto body = [&](auto odd) {
        for (int v = tid; v < (PX >> 1) * 8; v += 256) {
          const int p = v >> 3, cv = v & 7, ow = j0 - 2 + 2 * p;
          Vec16<bf16_t> o[2];
          o[0].raw = u32x4{0u, 0u, 0u, 0u}; o[1].raw = o[0].raw;
          if (rok && ow >= 0 && ow < Wo) {                        // Wo is even: ow + 1 < Wo too
            const int yo = (((b * Ho + oh) * Wo + ow) * 64 + cv * 8) * 2;
            Vec16<bf16_t> yy[2];
            yy[0].raw = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsY, yo, 0, 0));
            yy[1].raw = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsY, yo + 128, 0, 0));
            float g8[2][8];
            stem_route_pair_buf<decltype(odd)::value>(rsP, rsI, yy, f_sc, f_sh, b, oh, ow >> 1, cv * 8, Hp, Wp, g8);
#pragma unroll
            for (int q2 = 0; q2 < 2; ++q2)
#pragma unroll
              for (int j = 0; j < 8; ++j) o[q2].set(j, f_a[j] * g8[q2][j] + f_b[j] * yy[q2].get(j) + f_c[j]);   // = vqa_stem_bwd_apply
          }
#pragma unroll
          for (int q2 = 0; q2 < 2; ++q2) *reinterpret_cast<u32x4*>(dst + (2 * p + q2) * LDP + cv * 8) = o[q2].raw;
        }
      };
      if (oh & 1) body(std::true_type{});
      else body(std::false_type{});
    } else {
      constexpr int NV = 64 / VEC;
      for (int v = tid; v < PX * NV; v += 256) {
        const int x = v / NV, cv = v - x * NV, ow = j0 - 2 + x;
        u32x4 val = {0u, 0u, 0u, 0u};
        if (rok && ow >= 0 && ow < Wo) val = *reinterpret_cast<const u32x4*>(src + (((size_t)b * Ho + oh) * Wo + ow) * 64 + cv * VEC);
        *reinterpret_cast<u32x4*>(dst + x * LDP + cv * VEC) = val;
      }
    }
  };
  // ---- one finished quad row (staged in ost) -> the image, coalesced along W, masked at H-1 / W-1
  auto store = [&](int i) {
    for (int e = tid; e < 12 * SW; e += 256) {
      const int row = e / (2 * SW), col = e - row * 2 * SW, c = row >> 1, ih = 2 * i + (row & 1), iw = 2 * j0 + col;
      if (ih < H && iw < W) dimg[(((size_t)b * 3 + c) * H + ih) * W + iw] = ost[e];
    }
  };

  stage(i0 - 1); stage(i0); stage(i0 + 1);
  const int ntiles = SW / 16;
  for (int i = i0; i < i1; ++i) {
    if (i > i0) store(i - 1);
    stage(i + 2);
    __syncthreads();                                              // the four rows of quad row i are staged; ost has been stored
    for (int mt = wave; mt < ntiles; mt += 4) {
      // two accumulators (dy rows u = 0, 2 and u = 1, 3): independent MFMA chains (a single chain of 32 dependent MFMAs waits on the
      // accumulator latency; four chains cost the fused kernel its second workgroup per CU in registers); summed in a fixed order
      f32x4 accu[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
      const int jj = mt * 16 + li;                                // this lane's A row: quad column j0 + jj
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        f32x4 acc = accu[u & 1];
        const T* rowp = ring + ((i + u) & 3) * PX * LDP + (jj + 1) * LDP;     // dy row i-1+u, pixel ow = j0+jj-1 (+v)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          if constexpr (BF) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              const bf16x8 a = __builtin_bit_cast(bf16x8, *reinterpret_cast<const u32x4*>(rowp + v * LDP + h * 32 + g * 8));
              acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bw[(u * 4 + v) * 2 + h], acc, 0, 0, 0);
            }
          } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const f32x4 a = *reinterpret_cast<const f32x4*>(rowp + v * LDP + q * 16 + g * 4);
              const f32x4 w4 = *reinterpret_cast<const f32x4*>(bl + ((((u * 4 + v) * 4 + q) * 4 + g) * 16 + li) * 4);
#pragma unroll
              for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], w4[e], acc, 0, 0, 0);
            }
          }
        }
        accu[u & 1] = acc;
      }
      const f32x4 acc = accu[0] + accu[1];
      // D[row = quad 4g + r][col = n = li]
      if (li < 12) {
        const int c = li >> 2, ph = (li >> 1) & 1, pw = li & 1;
#pragma unroll
        for (int r = 0; r < 4; ++r) ost[(c * 2 + ph) * 2 * SW + 2 * (mt * 16 + 4 * g + r) + pw] = acc[r];
      }
    }
    __syncthreads();                                              // ost complete; ring slot of row i-1 free for row i+3
  }
  if (i1 > i0) store(i1 - 1);
}

extern "C" {

// packed data-gradient operand of the stem: dtype 1 (bf16) or 0 (fp32), 16*1024 elements
int vqa_stem_dgrad_pack(int dtype, const float* w_krsc, void* wpk, hipStream_t st) {
  if (!w_krsc || !wpk) return VQA_EARG;
  if (dtype) hipLaunchKernelGGL(stem_dgrad_pack_kernel<bf16_t>, dim3(16 * KTOT / 256), dim3(256), 0, st, w_krsc, (bf16_t*)wpk);
  else hipLaunchKernelGGL(stem_dgrad_pack_kernel<float>, dim3(16 * KTOT / 256), dim3(256), 0, st, w_krsc, (float*)wpk);
  VQA_LAUNCH_CHECK(); return VQA_OK;
}

int vqa_stem_dgrad_fused_ok(int B, int H, int W) {
  if (B <= 0 || H < 7 || W < 7) return 0;
  const int Ho = (H + 6 - 7) / 2 + 1, Wo = (W + 6 - 7) / 2 + 1;
  if (Wo & 1) return 0;                                           // staged in pixel pairs
  if ((size_t)B * Ho * Wo * 64 * 2 >= 0x7fffffffull) return 0;   // 32-bit buffer offsets (y; dpool and idx are smaller)
  return dg_shm<bf16_t>(dg_geom<bf16_t>(B, H, W).SW) <= (size_t)160 * 1024;
}

int vqa_stem_dgrad(int dtype, const void* dy, const void* wpk, float* dimg, int B, int H, int W, hipStream_t st) {
  if (!dy || !wpk || !dimg || B <= 0 || H < 7 || W < 7 || (long long)B * 3 * H * W >= (1ll << 40)) return VQA_EARG;
  if (dtype) {
    const DgGeom g = dg_geom<bf16_t>(B, H, W);
    const size_t shm = dg_shm<bf16_t>(g.SW);
    if (shm > 160 * 1024 || (long long)B * g.nband * g.nstrip >= 0x7fffffffll) return VQA_EARG;
    (void)vqa_ensure_lds(reinterpret_cast<const void*>(&stem_dgrad_kernel<bf16_t, false>), shm);
    hipLaunchKernelGGL((stem_dgrad_kernel<bf16_t, false>), dim3(B * g.nband * g.nstrip), dim3(256), shm, st, (const bf16_t*)dy,
                       (const bf16_t*)nullptr, (const uint8_t*)nullptr, (const float*)nullptr, (const float*)nullptr, (const bf16_t*)wpk,
                       dimg, B, H, W, g.Ho, g.Wo, 0, 0, g.SW, g.nstrip, g.QB, g.nband);
  } else {
    const DgGeom g = dg_geom<float>(B, H, W);
    const size_t shm = dg_shm<float>(g.SW);
    if (shm > 160 * 1024 || (long long)B * g.nband * g.nstrip >= 0x7fffffffll) return VQA_EARG;
    (void)vqa_ensure_lds(reinterpret_cast<const void*>(&stem_dgrad_kernel<float, false>), shm);
    hipLaunchKernelGGL((stem_dgrad_kernel<float, false>), dim3(B * g.nband * g.nstrip), dim3(256), shm, st, (const float*)dy,
                       (const bf16_t*)nullptr, (const uint8_t*)nullptr, (const float*)nullptr, (const float*)nullptr, (const float*)wpk,
                       dimg, B, H, W, g.Ho, g.Wo, 0, 0, g.SW, g.nstrip, g.QB, g.nband);
  }
  VQA_LAUNCH_CHECK(); return VQA_OK;
}

int vqa_stem_dgrad_fused(const void* y, const void* dpool, const uint8_t* idx, const float* coef, const float* bcoef, const void* wpk,
                         float* dimg, int B, int H, int W, hipStream_t st) {
  if (!y || !dpool || !idx || !coef || !bcoef || !wpk || !dimg || !vqa_stem_dgrad_fused_ok(B, H, W)) return VQA_EARG;
  const DgGeom g = dg_geom<bf16_t>(B, H, W);
  const int Hp = (g.Ho + 2 - 3) / 2 + 1, Wp = (g.Wo + 2 - 3) / 2 + 1;
  const size_t shm = dg_shm<bf16_t>(g.SW);
  (void)vqa_ensure_lds(reinterpret_cast<const void*>(&stem_dgrad_kernel<bf16_t, true>), shm);
  hipLaunchKernelGGL((stem_dgrad_kernel<bf16_t, true>), dim3(B * g.nband * g.nstrip), dim3(256), shm, st, (const bf16_t*)y,
                     (const bf16_t*)dpool, idx, coef, bcoef, (const bf16_t*)wpk, dimg, B, H, W, g.Ho, g.Wo, Hp, Wp, g.SW, g.nstrip, g.QB,
                     g.nband);
  VQA_LAUNCH_CHECK(); return VQA_OK;
}

}  // extern "C"
