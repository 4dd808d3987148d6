// MXFP8 (OCP Microscaling v1.0: e4m3fn elements, one E8M0 scale per 32 consecutive elements of the contraction axis) inference
// kernels for the Conv+BN-folded eval path of the residual blocks (gfx950 block-scaled MFMA):
//   mx_quant_kernel        : bf16 / fp32 [M][C] -> e4m3 codes [M][C] + E8M0 codes [M][C/32]
//   fold_bn_mxfp8_kernel   : eval-mode Conv+BN fold of every residual-block conv (vqa_fold_bn_batch's arithmetic) + quantization
//   conv_mxfp8_kernel      : NHWC implicit-GEMM conv on v_mfma_scale_f32_32x32x64_f8f6f4, vqa_igemm's bias / ReLU / addend epilogue,
//                            bf16 output and / or its MXFP8 copy
//
// The one quantization rule (pinned bit-exactly by tests/test_mxfp8_cpu.py and tests/test_gpu_mxfp8.py), per block of 32 values x_i:
//   amax = max |x_i| on the value as stored;  amax == 0 -> scale code 127, elements +0;
//   amax finite > 0 -> X = clamp(floor(log2 amax) - 8, -127, 127), scale code X + 127, q_i = e4m3fn_RNE(clamp(x_i / 2^X, -448, 448));
//   any x_i Inf / NaN -> scale code 0xFF (E8M0 NaN) and every element 0x7F (e4m3 NaN), so a consumer reads NaN through either.
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(8))) int i32x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;

// |v| as bits: for non-negative floats the unsigned order is the float order, and Inf / NaN (>= 0x7f800000) sort above every
// finite value, so one integer max finds amax AND whether the block holds a non-finite value.
__device__ __forceinline__ uint32_t mx_absbits(float v) { return __float_as_uint(v) & 0x7fffffffu; }

// max over aligned groups of G lanes (G a power of two <= 32)
template <int G>
__device__ __forceinline__ uint32_t mx_group_max(uint32_t b) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) {
    const uint32_t t = (uint32_t)__shfl_xor((int)b, o, 64);
    b = t > b ? t : b;
  }
  return b;
}

__device__ __forceinline__ int mx_scale_code(uint32_t amax_bits) {
  if (amax_bits >= 0x7f800000u) return 255;
  if (amax_bits == 0u) return 127;
  // floor(log2 amax): the exponent field for a normal amax; a subnormal amax (field 0) is below 2^-126, so X clamps to -127 anyway
  const int e = (int)(amax_bits >> 23) - 127;
  int x = e - 8;
  x = x < -127 ? -127 : (x > 127 ? 127 : x);
  return x + 127;
}

// e4m3fn code of v / 2^X (X = scode - 127), saturated to +-448, round to nearest even.  amax_bits == 0 gives +0.
__device__ __forceinline__ uint32_t mx_e4m3(float v, int scode, uint32_t amax_bits) {
  if (scode == 255) return 0x7fu;
  if (amax_bits == 0u) return 0u;
  // X is in [-127, 119] (amax < 2^128), so 2^-X is a normal float and the product is exact (a power-of-two scaling)
  const float y = v * __uint_as_float((uint32_t)(254 - scode) << 23);
  const uint32_t sign = (__float_as_uint(y) >> 24) & 0x80u;
  const float a = fminf(fabsf(y), 448.f);
  uint32_t code;
  if (a < 0.015625f) {                                   // below 2^-6: subnormal step 2^-9 (a code of 8 is the smallest normal)
    code = (uint32_t)rintf(a * 512.f);
  } else {
    const int e = (int)(__float_as_uint(a) >> 23) - 127;     // -6 .. 8
    const uint32_t m = (uint32_t)rintf(a * __uint_as_float((uint32_t)(130 - e) << 23));   // a * 2^(3-e) in [8, 16]
    code = ((uint32_t)(e + 7) << 3) + (m - 8u);              // m == 16 carries into the exponent; a <= 448 stays <= 0x7e
  }
  return sign | code;
}

// ---------------------------------------------------------------------------------------------------------------------------
// quantizer: 8 consecutive elements per thread, 4 lanes per 32-element block
// ---------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void mx_quant_kernel(const T* __restrict__ in, uint8_t* __restrict__ q, uint8_t* __restrict__ sc,
                                                        size_t n8) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= n8) return;                                   // n8 % 4 == 0: a block's four lanes leave together
  float v[8];
  if constexpr (sizeof(T) == 2) {
    const Vec16<T> x = ldg16(in + t * 8);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = x.get(i);
  } else {
    const Vec16<T> x0 = ldg16(in + t * 8), x1 = ldg16(in + t * 8 + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[i] = x0.get(i); v[4 + i] = x1.get(i); }
  }
  uint32_t mb = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) { const uint32_t b = mx_absbits(v[i]); mb = b > mb ? b : mb; }
  mb = mx_group_max<4>(mb);
  const int s = mx_scale_code(mb);
  uint32_t lo = 0, hi = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    lo |= mx_e4m3(v[i], s, mb) << (8 * i);
    hi |= mx_e4m3(v[4 + i], s, mb) << (8 * i);
  }
  *reinterpret_cast<uint2*>(q + t * 8) = make_uint2(lo, hi);
  if ((threadIdx.x & 3) == 0) sc[t >> 2] = (uint8_t)s;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Conv+BN fold + quantization: vqa_fold_bn_batch's table, grid and fp32 arithmetic; one element per thread, a 32-lane group per block
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fold_bn_mxfp8_kernel(const float* __restrict__ flat, uint8_t* __restrict__ wq, uint8_t* __restrict__ ws,
                                                             float* __restrict__ bout, const long long* __restrict__ desc, int nd, float eps) {
  int lo = 0, hi = nd - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (desc[(size_t)mid * 10 + 9] <= (long long)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const long long* d = desc + (size_t)lo * 10;
  const float* w = flat + d[0];
  const float* gamma = flat + d[1];
  const float* beta = flat + d[2];
  const float* rm = reinterpret_cast<const float*>(d[3]);
  const float* rv = reinterpret_cast<const float*>(d[4]);
  const int N = (int)d[5], K = (int)d[6];
  // table contract (the host wrapper checks it; this keeps a bad piece from racing on shared scale bytes or shuffling with exited
  // lanes): dst_off % 32 == 0 and K % 32 == 0.  A piece that breaks it is left unwritten -- uniform for the whole workgroup.
  if (((d[7] | (long long)K) & 31) != 0) return;
  const size_t i = (size_t)(blockIdx.x - (int)d[9]) * blockDim.x + threadIdx.x;
  if (i >= (size_t)N * K) return;                        // N * K % 32 == 0: a 32-element block leaves as a whole
  const int n = (int)(i / K);
  const float sc = gamma[n] / sqrtf(rv[n] + eps);
  const float v = w[i] * sc;
  const uint32_t mb = mx_group_max<32>(mx_absbits(v));
  const int s = mx_scale_code(mb);
  wq[d[7] + i] = (uint8_t)mx_e4m3(v, s, mb);
  if ((threadIdx.x & 31) == 0) ws[(d[7] + i) >> 5] = (uint8_t)s;
  if (i < (size_t)N) {
    const float s2 = gamma[i] / sqrtf(rv[i] + eps);
    bout[d[8] + i] = beta[i] - rm[i] * s2;
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// implicit-GEMM conv: out[M][N] = gather(A)[M][K] . W[N][K]^T, K = R*S*C ordered (tap, channel) like the folded weights
// ---------------------------------------------------------------------------------------------------------------------------
struct MxConvParams {
  const uint8_t* a; const uint8_t* as;         // activation codes [B*H*W][C], scales [B*H*W][C/32]
  const uint8_t* w; const uint8_t* ws;         // weight codes [N][K], scales [N][K/32]
  const float* bias; const bf16_t* addend;     // [N] fp32, [M][N] bf16 (either may be null)
  bf16_t* out; uint8_t* oq; uint8_t* os;       // bf16 [M][N] and / or its MXFP8 copy [M][N] + [M][N/32]
  int M, N, K, H, W, C, Ho, Wo, S, stride, pad, relu;
};

constexpr int MX_BM = 128, MX_BK = 128, MX_LD = MX_BK + 16;   // 144-byte LDS rows: 8 lanes' 16-byte reads hit 8 distinct bank quads

// What a loader lane reads when its operand is not there (zero-padding halo, rows past M, the empty half of K's last step): 64 zero
// codes and two unit scales (E8M0 127).  Every load is then unconditional -- a per-element "load or constant" select makes hipcc
// branch around each load -- and only the ADDRESS is selected.
__device__ __attribute__((aligned(16))) uint8_t mx_zero_codes[64];
__device__ __attribute__((aligned(4))) uint16_t mx_unit_scales[2] = {0x7f7f, 0x7f7f};

// 4 waves, 128 x BN tile, BK = 128 (two 64-deep MFMA steps per barrier pair).  Wave grid WM x WN, each wave 32*MT rows x 64 columns.
// Block-scaled MFMA 32x32x64, e4m3 x e4m3, maps measured with exact data: lane l (r = l & 31, h = l >> 5) holds row r of A in its
// 8 VGPRs, and the E8M0 scale in byte 0 of lane r's scale VGPR covers bytes 0..15 of lanes r AND r + 32, lane r + 32's scale bytes
// 16..31 of both.  So with a 64-deep step = two MX blocks, lane half h takes elements 16h .. 16h+15 of block 0 in bytes 0..15 and
// the same elements of block 1 in bytes 16..31, and its scale is block h's.  B the same with column r.  D: the standard
// 32x32 map, column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5): the 32 lanes of a half hold 32 consecutive output
// channels of one pixel -- exactly one MXFP8 block of the output, quantized with shuffles in the epilogue.
// Global -> register prefetch of step t+1 runs under the MFMAs of step t; registers -> LDS between two barriers.  (A two-stage LDS
// ring with one barrier per step measured slower: 0.43x instead of 0.56x the bf16 launch on stage 1 -- it halves the workgroups
// per CU -- so it is not used.)
template <int BN>
__global__ __launch_bounds__(256) void conv_mxfp8_kernel(MxConvParams p) {
  constexpr int WN = BN / 64, WM = 4 / WN, RW = MX_BM / WM, MT = RW / 32, NT = 2;
  __shared__ __attribute__((aligned(16))) uint8_t smem[(MX_BM + BN) * MX_LD + (MX_BM + BN) * 4];
  uint8_t* As = smem;
  uint8_t* Bs = smem + MX_BM * MX_LD;
  uint8_t* Asc = smem + (MX_BM + BN) * MX_LD;
  uint8_t* Bsc = Asc + MX_BM * 4;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  const int m0 = blockIdx.x * MX_BM, n0 = blockIdx.y * BN;

  // loader: thread -> (tile row tid >> 1, 64-byte half tid & 1 of the 128-deep step): 64 bytes of A, of B, two scale bytes each
  const int lrow = tid >> 1, lsub = tid & 1;
  const int m = m0 + lrow;
  const bool mval = m < p.M;
  int hb = 0, wb = 0;
  size_t pixb = 0;
  if (mval) {
    const int hw = p.Ho * p.Wo, b = m / hw, r = m - b * hw, ho = r / p.Wo, wo = r - ho * p.Wo;
    hb = ho * p.stride - p.pad; wb = wo * p.stride - p.pad;
    pixb = (size_t)b * p.H * p.W;
  }
  const bool bload = lrow < BN;
  const int cb = p.C >> 5, kb = p.K >> 5;
  const uint8_t* wrow = p.w + (size_t)(n0 + (bload ? lrow : 0)) * p.K;
  const uint8_t* wsrow = p.ws + (size_t)(n0 + (bload ? lrow : 0)) * kb;
  const int nk = (p.K + MX_BK - 1) / MX_BK;

  u32x4 ra[4], rb[4];
  uint32_t rsa, rsb;
  auto load = [&](int kt) {
    const int k = kt * MX_BK + lsub * 64;
    const bool kv = k < p.K;                             // K % 128 == 64 (stage 1, 3x3): the last step's second half is empty
    const int tap = k / p.C, c0 = k - tap * p.C, r = tap / p.S, s = tap - r * p.S;
    const int hi = hb + r, wi = wb + s;
    // zero-padding halo, rows past M, K past its end: the zero page (zeros with a finite scale)
    const bool av = mval && kv && (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W;
    const size_t pix = pixb + (size_t)hi * p.W + wi;
    const uint8_t* src = av ? p.a + pix * p.C + c0 : mx_zero_codes;
    const uint8_t* ssrc = av ? p.as + pix * cb + (c0 >> 5) : reinterpret_cast<const uint8_t*>(mx_unit_scales);
    const bool bv = bload && kv;
    const uint8_t* wsrc = bv ? wrow + k : mx_zero_codes;
    const uint8_t* wssrc = bv ? wsrow + (k >> 5) : reinterpret_cast<const uint8_t*>(mx_unit_scales);
#pragma unroll
    for (int q = 0; q < 4; ++q) ra[q] = *reinterpret_cast<const u32x4*>(src + 16 * q);
    rsa = *reinterpret_cast<const uint16_t*>(ssrc);
#pragma unroll
    for (int q = 0; q < 4; ++q) rb[q] = *reinterpret_cast<const u32x4*>(wsrc + 16 * q);
    rsb = *reinterpret_cast<const uint16_t*>(wssrc);
  };

  f32x16 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int h = lane >> 5, r32 = lane & 31;
  load(0);
  for (int kt = 0; kt < nk; ++kt) {
    __syncthreads();                                     // the previous step's fragments are read
    {
      uint8_t* da = As + lrow * MX_LD + lsub * 64;
#pragma unroll
      for (int q = 0; q < 4; ++q) *reinterpret_cast<u32x4*>(da + 16 * q) = ra[q];
      *reinterpret_cast<uint16_t*>(Asc + lrow * 4 + lsub * 2) = (uint16_t)rsa;
      if (bload) {
        uint8_t* db = Bs + lrow * MX_LD + lsub * 64;
#pragma unroll
        for (int q = 0; q < 4; ++q) *reinterpret_cast<u32x4*>(db + 16 * q) = rb[q];
        *reinterpret_cast<uint16_t*>(Bsc + lrow * 4 + lsub * 2) = (uint16_t)rsb;
      }
    }
    __syncthreads();
    if (kt + 1 < nk) load(kt + 1);
    const int ksteps = (p.K - kt * MX_BK) >= MX_BK ? 2 : 1;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      if (ks >= ksteps) break;
      i32x8 af[MT], bf[NT];
      int sa[MT], sb[NT];
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        const int row = wm * RW + i * 32 + r32;
        const uint8_t* s = As + row * MX_LD + ks * 64 + h * 16;
        const u32x4 x0 = *reinterpret_cast<const u32x4*>(s), x1 = *reinterpret_cast<const u32x4*>(s + 32);
        af[i] = i32x8{(int)x0[0], (int)x0[1], (int)x0[2], (int)x0[3], (int)x1[0], (int)x1[1], (int)x1[2], (int)x1[3]};
        sa[i] = Asc[row * 4 + ks * 2 + h];
      }
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        const int col = wn * 64 + j * 32 + r32;
        const uint8_t* s = Bs + col * MX_LD + ks * 64 + h * 16;
        const u32x4 x0 = *reinterpret_cast<const u32x4*>(s), x1 = *reinterpret_cast<const u32x4*>(s + 32);
        bf[j] = i32x8{(int)x0[0], (int)x0[1], (int)x0[2], (int)x0[3], (int)x1[0], (int)x1[1], (int)x1[2], (int)x1[3]};
        sb[j] = Bsc[col * 4 + ks * 2 + h];
      }
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(af[i], bf[j], acc[i][j], 0, 0, 0, sa[i], 0, sb[j]);
    }
  }

  // ---- epilogue (vqa_igemm's order): + bias, relu 1, bf16 round, + addend, bf16 round, relu 2; then the bf16 and / or MXFP8 stores
  const int nb32 = p.N >> 5;
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int n = n0 + wn * 64 + j * 32 + r32;
    const float bv = p.bias ? p.bias[n] : 0.f;
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int mm = m0 + wm * RW + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        const bool live = mm < p.M;                      // uniform over the 32-lane half (one pixel)
        const size_t off = (size_t)mm * p.N + n;
        float v = acc[i][j][r] + bv;
        if (p.relu == 1 && v < 0.f) v = 0.f;             // NaN-propagating, like torch
        v = bf2f(f2bf(v));
        if (p.addend) {
          const float ad = live ? bf2f(p.addend[off]) : 0.f;
          v = bf2f(f2bf(v + ad));
        }
        if (p.relu == 2 && v < 0.f) v = 0.f;
        if (live && p.out) p.out[off] = f2bf(v);
        if (p.oq) {                                      // quantized from the bf16 value just stored: = vqa_mx_quant(out)
          const uint32_t mb = mx_group_max<32>(mx_absbits(v));
          const int s = mx_scale_code(mb);
          if (live) {
            p.oq[off] = (uint8_t)mx_e4m3(v, s, mb);
            if (r32 == 0) p.os[(size_t)mm * nb32 + (n >> 5)] = (uint8_t)s;
          }
        }
      }
  }
}

}  // namespace

extern "C" {

// in: bf16 (dtype 1) or fp32 (dtype 0) [M][C], C % 32 == 0 -> q: e4m3 codes [M][C], s: E8M0 codes [M][C/32]
int vqa_mx_quant(int dtype, const void* in, uint8_t* q, uint8_t* s, int M, int C, hipStream_t st) {
  if (!in || !q || !s || M <= 0 || C <= 0 || (C % 32) != 0 || (dtype != 0 && dtype != 1)) return VQA_EARG;
  const size_t n8 = (size_t)M * C / 8;
  const dim3 grid((unsigned)((n8 + 255) / 256));
  if (dtype) hipLaunchKernelGGL(mx_quant_kernel<bf16_t>, grid, dim3(256), 0, st, (const bf16_t*)in, q, s, n8);
  else hipLaunchKernelGGL(mx_quant_kernel<float>, grid, dim3(256), 0, st, (const float*)in, q, s, n8);
  VQA_LAUNCH_CHECK();
  return VQA_OK;
}

// vqa_fold_bn_batch's table and grid; the folded fp32 weight of piece d is quantized to wq[dst_off ...] (codes) and
// ws[dst_off / 32 ...] (scales): every dst_off and N * K must be a multiple of 32.  bout as vqa_fold_bn_batch.
int vqa_fold_bn_mxfp8(const float* flat, uint8_t* wq, uint8_t* ws, float* bout, const long long* desc, int nd, int total_blocks, float eps,
                      hipStream_t st) {
  if (!flat || !wq || !ws || !bout || !desc || nd <= 0 || total_blocks <= 0) return VQA_EARG;
  hipLaunchKernelGGL(fold_bn_mxfp8_kernel, dim3(total_blocks), dim3(256), 0, st, flat, wq, ws, bout, desc, nd, eps);
  VQA_LAUNCH_CHECK();
  return VQA_OK;
}

int vqa_conv_mxfp8(const uint8_t* a, const uint8_t* as, const uint8_t* w, const uint8_t* ws, const float* bias, const void* addend,
                   void* out, uint8_t* oq, uint8_t* os, int M, int N, int B, int H, int W, int C, int Ho, int Wo, int R, int S,
                   int stride, int pad, int relu, hipStream_t st) {
  if (!a || !as || !w || !ws || (!out && !oq) || (!oq) != (!os)) return VQA_EARG;
  if (M <= 0 || B <= 0 || H <= 0 || W <= 0 || C <= 0 || (C % 64) != 0 || N <= 0 || (N % 64) != 0) return VQA_EARG;
  if (R != S || !((R == 3 && pad == 1) || (R == 1 && pad == 0)) || (stride != 1 && stride != 2) || relu < 0 || relu > 2) return VQA_EARG;
  if (Ho != (H + 2 * pad - R) / stride + 1 || Wo != (W + 2 * pad - S) / stride + 1 || (long long)M != (long long)B * Ho * Wo) return VQA_EARG;
  if ((long long)M * N >= (1ll << 31) || (long long)B * H * W * C >= (1ll << 31)) return VQA_EARG;
  MxConvParams p;
  p.a = a; p.as = as; p.w = w; p.ws = ws; p.bias = bias; p.addend = (const bf16_t*)addend;
  p.out = (bf16_t*)out; p.oq = oq; p.os = os;
  p.M = M; p.N = N; p.K = R * S * C; p.H = H; p.W = W; p.C = C; p.Ho = Ho; p.Wo = Wo; p.S = S;
  p.stride = stride; p.pad = pad; p.relu = relu;
  const unsigned mt = (unsigned)((M + MX_BM - 1) / MX_BM);
  if (N % 128 == 0) hipLaunchKernelGGL(conv_mxfp8_kernel<128>, dim3(mt, N / 128), dim3(256), 0, st, p);
  else hipLaunchKernelGGL(conv_mxfp8_kernel<64>, dim3(mt, N / 64), dim3(256), 0, st, p);
  VQA_LAUNCH_CHECK();
  return VQA_OK;
}

}  // extern "C"
