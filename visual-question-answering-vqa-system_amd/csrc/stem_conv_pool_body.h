// Body of stem_conv_pool_kernel and stem_conv_pool_u8_kernel (stem_conv.hip includes it inside both, with SRC = ImgF32 / ImgU8 and
// `img`, `tab` and the kernel's other parameters in scope).  The other two stem kernels share a __device__ body templated on the image
// source; this one keeps its text inside the __global__ function because, inlined from a __device__ template, the fp32 kernel compiled
// to other code (213 instead of 215 VGPRs, 3080 instead of 3386 instructions) and the fp32 kernels are to stay what they were.
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* patch = reinterpret_cast<bf16_t*>(smem);                 // [3][PRP][PW], x = iw + 5
  bf16_t* Wl = patch + 3 * PRP * PW;                                // [64][LDW]
  bf16_t* Cst = Wl;                                                 // [4 waves][8][LDCS] once the B fragments are in registers
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
  const int pblocks = Hp / PRB;
  const int b = blockIdx.x / pblocks, ph0 = (blockIdx.x - b * pblocks) * PRB;

  for (int v = tid; v < 64 * (KP / 8); v += 256) {
    const int n = v / (KP / 8), kv = v - n * (KP / 8);
    *reinterpret_cast<u32x4*>(&Wl[n * LDW + kv * 8]) = *reinterpret_cast<const u32x4*>(&wst[n * KP + kv * 8]);
  }
  const int ih_base = 4 * ph0 - 5;                                   // input row of patch row 0: 2 * (2 * ph0 - 1) - 3
  const SRC src(img, tab, B * 3 * H * W);
  if (dbg & 8) {}
  else if (!(W & 3)) stem_fill_vec<PRP, 5>(patch, PW, src, b, ih_base, H, W, tid);
  else
  for (int x = tid; x < PW; x += 256) {
    const int iw = x - 5;
    const bool cok = iw >= 0 && iw < W;
    const int iwc = min(max(iw, 0), W - 1);
#pragma unroll
    for (int c = 0; c < 3; ++c) {                                    // one channel's 23 rows in flight at a time
      typename SRC::raw_t vals[PRP];
#pragma unroll
      for (int pr = 0; pr < PRP; ++pr) {
        const int ih = ih_base + pr;
        const int ihc = min(max(ih, 0), H - 1);
        vals[pr] = SRC::pick(cok && ih >= 0 && ih < H, src.load(b, c, ihc, iwc, H, W));
      }
#pragma unroll
      for (int pr = 0; pr < PRP; ++pr) patch[(c * PRP + pr) * PW + x] = src.bits(vals[pr], c);
    }
  }
  __syncthreads();
  bf16x8 bfr[6][4];
#pragma unroll
  for (int kk = 0; kk < 6; ++kk)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
      bfr[kk][nt] = *reinterpret_cast<const bf16x8*>(&Wl[(nt * 16 + li) * LDW + kk * 32 + g * 8]);
  float sc[4], sh[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) { sc[nt] = coef[nt * 16 + li]; sh[nt] = coef[64 + nt * 16 + li]; }
  __syncthreads();                                                   // Wl is dead: C staging may overwrite it
  if (dbg & 4) { if (tid == 0) out[(size_t)blockIdx.x * 64] = f2bf(sc[0] + (float)bfr[0][0][0]); return; }

  bf16_t* mycs = Cst + wave * 8 * LDCS;
  for (int t = wave; t < ctiles; t += 4) {
    const int c0 = 14 * t - 1;                                        // conv column of accumulator row p = 0
    // conv row i of the block (conv row 2*ph0 - 1 + i) -> BN + ReLU -> horizontal 3-max at stride 2: h[nt][0] = pooled column 2g,
    // h[nt][1] = pooled column 2g + 1 (garbage for g == 3: never stored)
    auto row = [&](int i, float (&h)[4][2]) {
      f32x4 acc[4];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (!(dbg & 1))
#pragma unroll
      for (int kk = 0; kk < 6; ++kk) {
        int pair = kk * 4 + g;
        pair = pair > 20 ? 20 : pair;
        const int c = pair / 7, r = pair - c * 7;
        const uint32_t* ap = reinterpret_cast<const uint32_t*>(&patch[(c * PRP + 2 * i + r) * PW + 28 * t + 2 * li]);
        u32x4 raw = {ap[0], ap[1], ap[2], ap[3] & 0x0000ffffu};       // s8 = 7 is padding: its pixel is the window's neighbour, and 0 * NaN is NaN
        const bf16x8 af = __builtin_bit_cast(bf16x8, raw);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bfr[kk][nt], acc[nt], 0, 0, 0);
      }
      if (dbg & 2) {
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) { h[nt][0] = acc[nt][0] + acc[nt][1]; h[nt][1] = acc[nt][2] + acc[nt][3]; }
        return;
      }
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        float v[4];
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          const int col = c0 + 4 * g + r4;
          const float a = acc[nt][r4] * sc[nt] + sh[nt];
          v[r4] = ((unsigned)col < (unsigned)Wo) ? (a < 0.f ? 0.f : a) : 0.f;
        }
        const float nx = __shfl_down(v[0], 16, 64);                   // column 4g + 4
        h[nt][0] = pool_max(pool_max(v[0], v[1]), v[2]);
        h[nt][1] = pool_max(pool_max(v[2], v[3]), nx);
      }
    };
    float hp[4][2], h1[4][2], h2[4][2];
    if (ph0 > 0) row(0, hp);                                          // conv row 2*ph0 - 1 (row -1 of the image: outside)
    else {
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) { hp[nt][0] = 0.f; hp[nt][1] = 0.f; }
    }
#pragma unroll 1
    for (int k = 0; k < PRB; ++k) {
      row(2 * k + 1, h1);
      row(2 * k + 2, h2);
      // this lane's two pooled columns x four channel tiles -> wave-private staging -> 16-byte row stores
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const float o = pool_max(pool_max(hp[nt][q], h1[nt][q]), h2[nt][q]);
          mycs[(2 * g + q) * LDCS + nt * 16 + li] = f2bf(o);
          hp[nt][q] = h2[nt][q];
        }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      const int px = lane >> 3, cv = lane & 7, pw = 7 * t + px;
      if (px < 7 && pw < Wp)
        *reinterpret_cast<u32x4*>(&out[((((size_t)b * Hp + ph0 + k) * Wp + pw) * 64) + cv * 8]) = *reinterpret_cast<const u32x4*>(&mycs[px * LDCS + cv * 8]);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
  }
