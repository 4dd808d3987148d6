/* libvqa_hip.so -- C ABI of the MI355X (gfx950) VQA forward/backward kernels.
 *
 * Conventions:
 *   - raw DEVICE pointers + explicit sizes + a hipStream_t; the caller (PyTorch) owns every buffer, including
 *     workspaces and tensors saved for backward; functions never allocate, never synchronise, never throw;
 *   - return value: 0 = launched, 1000 = argument/shape error (nothing launched), otherwise a hipError_t;
 *   - dtype: 0 = float32 (fp32 MFMA, parity path), 1 = bfloat16 (bf16 MFMA, fp32 accumulate); statistics,
 *     coefficients, weight gradients and optimizer state are always float32;
 *   - CNN activations are NHWC, token tensors are [rows][D]; conv weights are [Cout][R][S][Cin];
 *   - "+=" outputs (weight / bias gradients) accumulate into caller-zeroed fp32 buffers;
 *   - entries read only the stated extent of each operand and write only their outputs and the reported scratch.
 * Each entry cites the reference interface (path relative to the reference checkout) it replaces.
 */
#ifndef VQA_HIP_H
#define VQA_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
typedef struct ihipStream_t* hipStream_t;

/* ---- implicit-GEMM convolution / linear -------------------------------------------------------------------
 * Replaces nn.Conv2d forward + its autograd backward (models/cnn_backbone.py:148-158 conv1/conv2, :243-247 shortcut,
 * :350 stem) and every nn.Linear (models/text_encoder.py:176-179,309-310; models/cross_attention.py:98-101,257-263;
 * models/fusion.py:68; models/vqa_model.py:74-82).
 * loader 0: NHWC activations, 1: 7x7/2 stem straight from the NCHW fp32 image.
 * out[M][N] = gather(a)[M][Kw] * w[N][Kw]^T, then +bias, ReLU, dropout(drop_p, drop_seed), + addend*(addmask>0);
 * stats != NULL: per-M-tile column sums / sums of squares ([vqa_igemm_mtiles][2][N]) for train-mode BatchNorm.
 * transposed = 1 gathers for the data gradient (a = dY [B,H,W,C], rows index dX [B,Ho,Wo]). */
int vqa_igemm_mtiles(int M, int N, int loader);
/* which template instantiation vqa_igemm launches for this problem (host-only query, no launch):
 * BM*10000 + BN*10 + flavour (0 plain LDS-DMA double buffer, 1 window loader) */
int vqa_igemm_variant(int dtype, int loader, int M, int N, int Kw, int B, int H, int W, int C, int Ho, int Wo,
                      int R, int S, int stride, int pad);
int vqa_igemm(int dtype, int loader, const void* a, const void* w, void* out, const float* bias, const void* addend,
              const void* addmask, const void* outmask /* out *= (outmask > 0), applied last */, float* stats, int M, int N, int Kw, int B, int H, int W, int C, int Ho, int Wo,
              int R, int S, int stride, int pad, int transposed, int relu, float drop_p, unsigned long long drop_seed,
              int stats_mode /* 0: stats = float slab [mtiles][2][N]; 1: stats = fixed-point accumulator (see vqa_bn_apply_acc) */,
              hipStream_t stream);
/* Data gradient of a Linear whose INPUT was relu(+dropout(p)) of the previous Linear, with the consumer's mask applied by the producer
 * (round 4): dx[M][Kin] = (dz[M][N] * wt[Kin][N]^T + addend) * (outact > 0) / (1 - drop_p); the keep scale multiplies the
 * value already rounded to the compute dtype, so dx is bit-equal to vqa_igemm followed by vqa_bias_act_bwd(outact, p).  Replaces the
 * autograd nodes of nn.ReLU + nn.Dropout between two nn.Linear (models/text_encoder.py:309-317 FeedForward, models/cross_attention.py:257-263,
 * models/vqa_model.py:74-82 AnswerHead).  wt = the [Kin][N] transposed weight (vqa_pack_transpose).  outact required. */
int vqa_linear_dgrad_act(int dtype, const void* dz, const void* wt, void* dx, const void* addend, const void* outact, float drop_p,
                         int M, int Kin, int N, hipStream_t stream);
/* dw[N][Kw] += dy[M][N]^T * gather(x)[M][Kw], split over the M pixels.
 * With a workspace (`ws`, caller-owned scratch of >= the ws_floats vqa_wgrad_plan reports; contents undefined afterwards) every
 * split writes its fp32 tile to its own slab and a second launch adds the slabs to dw in a FIXED order: dw is bit-reproducible,
 * no float atomics.  ws == NULL (or too small): fp32 atomics.  vqa_wgrad_plan is a host-only query: *kind 1 = the 8-wave LDS-DMA
 * kernel (bf16, the large CNN convs), 0 = the 4-wave kernel; tile, split count, workspace floats (0 = single split, no reduce). */
int vqa_wgrad_plan(int dtype, int loader, int M, int N, int Kw, int B, int H, int W, int C, int R, int S, long long* ws_floats,
                   int* kind, int* tile_n, int* tile_k, int* nsplit);
int vqa_wgrad(int dtype, int loader, const void* dy, const void* x, float* dw, int M, int N, int Kw, int B, int H, int W,
              int C, int Ho, int Wo, int R, int S, int stride, int pad, float* ws, long long ws_floats, hipStream_t stream);
int vqa_pack_rows(int dtype, const float* in, void* out, int N, int K, int Kp, hipStream_t stream);          /* cast + row pad   */
int vqa_pack_transpose(int dtype, const float* in, void* out, int N, int T, int C, int ldo, int col0, int flip, hipStream_t stream); /* out[c][col0+t*N+n] = in[n][flip?T-1-t:t][c] */
int vqa_pack_transpose_batch(int dtype, const float* flat, void* out, const long long* desc, int nd, int total_blocks, hipStream_t stream); /* nd pieces, device table desc[nd][10] = {src_off, dst_off, N, T, C, ldo, col0, flip, blk0, 0}, blk0 = running sum of T*ceil(N/32)*ceil(C/32): every data-gradient operand of a step in one launch */
/* Eval-mode Conv+BN folding, all convs in one launch (inference path, api/inference.py:196-323 via VQAModel.predict):
 * w'[n][k] = w[n][k]*gamma[n]/sqrt(running_var[n]+eps) cast to dtype, b'[n] = beta[n] - running_mean[n]*scale[n].
 * desc: device table [nd][10] int64 {w_off, gamma_off, beta_off (floats from flat), running_mean ptr, running_var ptr, N, K,
 * dst_off (elements of wout), bias_off (floats of bout), blk0}.  vqa_igemm's relu argument: 1 = ReLU before the addend,
 * 2 = ReLU after the addend (relu(conv + bias + residual)). */
int vqa_fold_bn_batch(int dtype, const float* flat, void* wout, float* bout, const long long* desc, int nd, int total_blocks, float eps, hipStream_t stream);
/* MXFP8 eval path of the residual blocks (csrc/mxfp8.hip).  MXFP8 = OCP e4m3fn element codes + one E8M0 scale code per 32
 * consecutive elements of the contraction axis (NHWC: 32 channels of one pixel; folded weights [Cout][R][S][Cin]: 32 input channels of
 * one tap).  Quantization rule: amax == 0 -> scale 127, elements +0; amax finite -> X = clamp(floor(log2 amax) - 8, -127, 127), scale
 * X + 127, q = e4m3fn RNE of clamp(x / 2^X, -448, 448); an Inf / NaN in the block -> scale 0xFF and every element 0x7F.
 * vqa_mx_quant: in bf16 (dtype 1) / fp32 (dtype 0) [M][C], C % 32 == 0 -> q [M][C], s [M][C/32].
 * vqa_fold_bn_mxfp8: vqa_fold_bn_batch's table and grid; codes at wq + dst_off, scales at ws + dst_off / 32 (dst_off % 32 == 0), bias as there.
 * vqa_conv_mxfp8: NHWC implicit-GEMM conv (3x3 pad 1 or 1x1 pad 0, stride 1 / 2, C % 64 == 0, N % 64 == 0) of MXFP8 a / as and
 * w / ws [N][R*S*C] with vqa_igemm's epilogue (bias fp32, bf16 addend, relu 1 before / 2 after the addend) into bf16 out and / or
 * its MXFP8 copy oq [M][N] / os [M][N/32] (= vqa_mx_quant of the bf16 result). */
int vqa_mx_quant(int dtype, const void* in, uint8_t* q, uint8_t* s, int M, int C, hipStream_t stream);
int vqa_fold_bn_mxfp8(const float* flat, uint8_t* wq, uint8_t* ws, float* bout, const long long* desc, int nd, int total_blocks, float eps,
                      hipStream_t stream);
int vqa_conv_mxfp8(const uint8_t* a, const uint8_t* as, const uint8_t* w, const uint8_t* ws, const float* bias, const void* addend,
                   void* out, uint8_t* oq, uint8_t* os, int M, int N, int B, int H, int W, int C, int Ho, int Wo, int R, int S,
                   int stride, int pad, int relu, hipStream_t stream);
/* stage-1 3x3/1 conv, 64->64 channels, bf16, LDS-resident input patch (models/cnn_backbone.py:182-187 at Cin=Cout=64): forward
 * (w = [Cout][R][S][Cin]) or data gradient (w = flipped+transposed pack) without epilogue inputs: 8-wave persistent kernel, 8 output rows per
 * block, input patches by LDS-DMA, weights in registers; stats [vqa_conv3x3_c64p_blocks][2][64] or NULL.  H % 8 == 0, W % 8 == 0. */
int vqa_conv3x3_c64p_blocks(int B, int H, int W);
/* ... and the data gradient of a residual block's conv1 (w = flipped + transposed pack) with the identity path in the epilogue:
 * out = (conv + addend * (addmask > 0)) * (outmask > 0) on the bf16 conv value, as vqa_igemm / vqa_conv8p; addend required, masks or NULL. */
/* ... and conv2's data gradient that also leaves bn1's BatchNorm-backward column sums (as vqa_conv8p's bn_y / bn_coef / bn_facc): the
 * stored tile is the gradient entering relu(BatchNorm(bn_y)); bn_coef = coef[4][64], bn_facc = zeroed vqa_bn_acc_words(3, 64). */
int vqa_conv3x3_c64p_bnred(const void* x, const void* w, void* out, const void* bn_y, const float* bn_coef, unsigned long long* bn_facc,
                           int B, int H, int W, hipStream_t stream);
int vqa_conv3x3_c64p_epi(const void* x, const void* w, void* out, const void* addend, const void* addmask, const void* outmask,
                         int B, int H, int W, hipStream_t stream);
int vqa_conv3x3_c64p(const void* x, const void* w, void* out, float* stats, int B, int H, int W,
                     int stats_mode /* 1: stats is the fixed-point accumulator u64 [2*64 + 1] of vqa_bn_apply_acc */, hipStream_t stream);
/* Round 4 -- the 256 x 256 x 64 8-phase GEMM core (csrc/gemm8p.hip): C[M][N] = A[M][K] . B[N][K]^T, bf16 operands, fp32 accumulation,
 * bf16 result; M % 256 == 0, N % 256 == 0, K % 64 == 0.  The dense form of the tile that vqa_conv8p runs as an implicit GEMM. */
int vqa_gemm8p(const void* A, const void* B, void* C, int M, int N, int K, hipStream_t stream);
/* the same product on the four-wave kernel (one wave per SIMD, 128 x 128 wave tiles in the accumulator registers; same shape rules) */
int vqa_gemm4w(const void* A, const void* B, void* C, int M, int N, int K, hipStream_t stream);
/* vqa_conv8p: the same tile as an implicit-GEMM 3x3 / stride 1 / pad 1 convolution over NHWC bf16 (models/cnn_backbone.py:182-187 at
 * 256 / 512 channels): out[B*H*W][N] = conv(x [B][H][W][C], w [N][(r, s, c)]) with transposed = 0; with transposed = 1 the stride-1 data
 * gradient (x = dy [B][H][W][Cout], w = the [Cin][(tap, Cout)] pack of vqa_pack_transpose, taps mirrored).  Tiles hold 196 valid output
 * pixels of 224 when 196 divides B*H*W (one 14 x 14 image / four 7 x 7 images: exactly 2 / 1 rounds of 256 CUs at B = 512).
 * stats: NULL, or the fixed-point BatchNorm accumulator (vqa_bn_acc_words(2, N), caller-zeroed) for sum y | sum y^2 of the stored values.
 * vqa_conv8p_ok: 1 when the shape is taken (C a power-of-two multiple of 64, N a multiple of 256). */
int vqa_conv8p_ok(int B, int H, int W, int C, int N);
int vqa_conv8p(const void* x, const void* w, void* out, unsigned long long* stats,
               const void* addend, const void* addmask, const void* outmask /* [B*H*W][N] bf16 or NULL: out = (conv + addend * (addmask > 0)) * (outmask > 0) */,
               const void* bn_y, const float* bn_coef, unsigned long long* bn_facc /* all or none: also the BatchNorm-backward column sums of the stored
                  tile as the gradient entering relu(BatchNorm(bn_y)): sum g | sum g*xhat, g = out * [bn_y*scale + shift > 0], into bn_facc
                  (vqa_bn_acc_words(3, N)); the caller then skips vqa_bn_bwd_reduce and runs vqa_bn_bwd_apply_acc on it */,
               int bn_selfmask /* 1: as above (ReLU directly behind that BatchNorm, mask recomputed from bn_y); 0: g = out, the tile already carries
                  its mask (outmask = the output of the block whose bn2 this is) */,
               const void* bn_y2, const float* bn_coef2 /* both or none, bn_selfmask 0 only: the 1x1 shortcut's BatchNorm sharing g -> third row
                  sum g*xhat(bn_y2), as vqa_bn_bwd_reduce with y2 / coef2 */,
               int B, int H, int W, int C, int N, int transposed, int stride /* 1, or 2: forward 3x3 / 2 convs (H, W = input map) */, hipStream_t stream);
/* Round 4 -- training-mode "Conv3x3 + BN + ReLU" without the normalised tensor (models/cnn_backbone.py:182-187: conv1 -> bn1 -> relu ->
 * conv2 at 64 channels).  vqa_conv3x3_c64p_bn is vqa_conv3x3_c64p applied to relu(BatchNorm(y)): y = the previous conv's raw output,
 * acc = its fixed-point statistics (the launch that wrote y ran with stats_mode = 1).  Every workgroup finalizes the 64 coefficients in
 * its prologue, workgroup 0 publishes coef_out[4][64] (scale | shift | mean | invstd) and updates the running statistics (what
 * vqa_bn_apply_acc does), and each input patch is normalised + ReLU'd IN LDS after its DMA landed -- zero padding stays zero; the conv
 * result is bit-identical to vqa_conv3x3_c64p(vqa_bn_apply_acc(y)).  vqa_wgrad3x3_c64_bn is the matching weight gradient
 * dw += dy^T gather(relu(y * coef[c] + coef[64 + c])) on the 8-wave kernel (vqa_wgrad3x3_c64_bn_ok: 1 when it takes the shape). */
int vqa_conv3x3_c64p_bn(const void* y, const unsigned long long* acc, const float* gamma, const float* beta, float* running_mean,
                        float* running_var, long long* num_batches_tracked, float* coef_out, const void* w, void* out, float* stats,
                        int B, int H, int W, int stats_mode, double count, float momentum, float eps, hipStream_t stream);
int vqa_wgrad3x3_c64_bn_ok(int B, int H, int W);
int vqa_wgrad3x3_c64_bn(const void* y, const float* coef, const void* dy, float* dw /* [64][576] += */, int B, int H, int W,
                        float* ws /* vqa_wgrad3x3_c64_blocks * 64*576 floats */, long long ws_floats, hipStream_t stream);
/* stage-2 weight gradient (3x3 / 1 / pad 1, 128 -> 128 channels, 28 x 28 maps, bf16; models/cnn_backbone.py:182-187 backward): 8-wave
   LDS-DMA kernel + fixed-order slab reduce.  vqa_wgrad3x3_c128_blocks: slabs of 128*576 floats the workspace must hold, 0 = shape not
   supported (the caller uses vqa_wgrad). */
int vqa_wgrad3x3_c128_blocks(int B, int H, int W);
int vqa_wgrad3x3_c128(const void* x, const void* dy, float* dw, int B, int H, int W, float* ws, long long ws_floats, hipStream_t stream);
int vqa_wgrad3x3_c64_blocks(int B, int H, int W);   /* [64][576] slabs of scratch vqa_wgrad3x3_c64 wants for this shape (0: unsupported) */
int vqa_wgrad3x3_c64(const void* x, const void* dy, float* dw /* [64][576] += */, int B, int H, int W,
                     float* ws /* >= vqa_wgrad3x3_c64_blocks * 64*576 floats of scratch, or NULL: 4-wave kernel with atomics */,
                     long long ws_floats, hipStream_t stream);
/* Up to 8 Linear weight gradients dw_j[N_j][K_j] += dy_j[M_j][N_j]^T x_j[M_j][K_j] in ONE launch + ONE fixed-order reduce launch
   (training/train.py:196 loss.backward() -> the token-side nn.Linear weights of models/text_encoder.py, cross_attention.py, fusion.py,
   answer_head.py).  Each dw_j is bit-identical to its own vqa_wgrad call.  vqa_wgrad_group_ws: floats of the shared workspace, or -1
   when a job is not one the planner gives the 4-wave 128x128 split kernel (the caller then uses vqa_wgrad). */
long long vqa_wgrad_group_ws(int dtype, int njobs, const int* M, const int* N, const int* Kw);
int vqa_wgrad_group(int dtype, int njobs, const void* const* dy, const void* const* x, float* const* dw, const int* M, const int* N,
                    const int* Kw, float* ws, long long ws_floats, hipStream_t stream);
/* second pass of the deterministic split weight gradients: dw[i] += sum_s ws[s][i] in slab order (n % 4 == 0) */
int vqa_slab_reduce(const float* ws, float* dw, int nslabs, long long n, hipStream_t stream);
/* data gradient of a stride-2 conv (+ the block's 1x1/2 shortcut, models/cnn_backbone.py:243-247) in one launch; rows are
 * grouped by output parity class so only the valid taps are issued.  dy/dyd [B][H][W][C], out [B][Ho=2H][Wo=2W][N] */
int vqa_dgrad_s2(int dtype, const void* dy, const void* dyd, const void* wt, void* out, int B, int H, int W, int C,
                 int Ho, int Wo, int N, int R, int pad, hipStream_t stream);
/* dedicated bf16 stem conv 7x7/2 (models/cnn_backbone.py:350): image patch + weights resident in LDS */
int vqa_stem_conv_blocks(int B, int H, int W);
int vqa_stem_pack(const float* w_krsc, void* wstem, hipStream_t stream);
int vqa_stem_conv(const float* img, const void* wstem, void* out, float* stats, int B, int H, int W, hipStream_t stream);
/* Inference stem in ONE launch: conv7x7/2 + BatchNorm with running statistics (coef = scale[64] | shift[64], vqa_bn_eval_coef) + ReLU +
   MaxPool3x3/2 p1 (models/cnn_backbone.py:349-354 in eval mode).  out: the pooled activation NHWC bf16 [B][Hp][Wp][64]; the conv
   output itself is never stored (no argmax either: no backward).  vqa_stem_conv_pool_ok: 1 when the shape is supported. */
int vqa_stem_conv_pool_ok(int B, int H, int W);
int vqa_stem_conv_pool(const float* img, const void* wstem, const float* coef, void* out, int B, int H, int W, hipStream_t stream);
int vqa_stem_wgrad_blocks(int B, int H, int W);   /* workgroups of the two stem weight-gradient kernels; their scratch: blocks * 64*147 floats */
int vqa_stem_wgrad(const float* img, const void* dy, float* dw /* [64][7][7][3] += */, int B, int H, int W,
                   float* ws /* scratch or NULL: atomics */, long long ws_floats, hipStream_t stream);
/* same, with the stem BN+ReLU+MaxPool backward apply fused in: dy is rebuilt per row from y, dpool, idx, coef, bcoef */
int vqa_stem_wgrad_fused(const float* img, const void* y, const void* dpool, const uint8_t* idx, const float* coef,
                         const float* bcoef, float* dw, int B, int H, int W, float* ws, long long ws_floats, hipStream_t stream);
/* The same four kernels fed from the uint8 HWC batch a decoder / the GPU input pipeline holds (img_hwc [B][H][W][3], a pixel at
 * ((b*H + ih)*W + iw)*3 + c; VQA_EARG from 2^31 - 1 bytes on): `table` is the bf16 [3][256] block vqa_u8_norm_table wrote,
 * table[c][v] = bf16((float(v)/255 - mean[c]) / std[c]) -- vqa_image_normalize's expression and the bf16 rounding the fp32 kernels
 * apply to their input -- so every output is bit-equal to the fp32 entry's on vqa_image_normalize's (unflipped) output.  The padding
 * outside the image is 0.0 in normalised space.  Same shapes, grids and scratch as the fp32 entries (the _blocks / _ok queries hold
 * for both).  vqa_u8_norm_table: one workgroup; VQA_EARG for a non-finite mean or a zero / non-finite std. */
int vqa_u8_norm_table(float mean0, float mean1, float mean2, float std0, float std1, float std2, void* table, hipStream_t stream);
int vqa_stem_conv_u8(const uint8_t* img_hwc, const void* wstem, void* out, float* stats, int B, int H, int W, const void* table,
                     hipStream_t stream);
int vqa_stem_conv_pool_u8(const uint8_t* img_hwc, const void* wstem, const float* coef, void* out, int B, int H, int W, const void* table,
                          hipStream_t stream);
int vqa_stem_wgrad_u8(const uint8_t* img_hwc, const void* dy, float* dw, int B, int H, int W, float* ws, long long ws_floats,
                      const void* table, hipStream_t stream);
int vqa_stem_wgrad_fused_u8(const uint8_t* img_hwc, const void* y, const void* dpool, const uint8_t* idx, const float* coef,
                            const float* bcoef, float* dw, int B, int H, int W, float* ws, long long ws_floats, const void* table,
                            hipStream_t stream);
/* Data gradient of the stem conv (the gradient with respect to the input image), an implicit GEMM over 2x2 image quads.  No atomics:
 * every image element is written exactly once (bit-reproducible).
 * vqa_stem_dgrad_pack: w_krsc [64][7][7][3] fp32 -> wpk, the packed [16][1024] operand in dtype (1: bf16, 0: fp32), 16*1024 elements.
 * vqa_stem_dgrad: dy [B][Ho][Wo][64] in dtype (as vqa_stem_bwd_apply writes it) -> dimg NCHW fp32 [B][3][H][W] (overwritten).
 *   Any H, W >= 7 the forward accepts; rows / columns past H-1 / W-1 are never written.
 * vqa_stem_dgrad_fused: bf16 only; dy is rebuilt from y [B][Ho][Wo][64], dpool [B][Hp][Wp][64], idx, coef (4*64) and bcoef (3*64)
 *   exactly as vqa_stem_bwd_apply computes it and never written.  vqa_stem_dgrad_fused_ok: 1 when the shape is supported (Wo even,
 *   B*Ho*Wo*64*2 bytes addressable with 32-bit buffer offsets); otherwise vqa_stem_dgrad_fused returns VQA_EARG and launches nothing. */
int vqa_stem_dgrad_pack(int dtype, const float* w_krsc, void* wpk, hipStream_t stream);
int vqa_stem_dgrad(int dtype, const void* dy, const void* wpk, float* dimg, int B, int H, int W, hipStream_t stream);
int vqa_stem_dgrad_fused_ok(int B, int H, int W);
int vqa_stem_dgrad_fused(const void* y, const void* dpool, const uint8_t* idx, const float* coef, const float* bcoef, const void* wpk,
                         float* dimg, int B, int H, int W, hipStream_t stream);

/* ---- BatchNorm2d (nn.BatchNorm2d defaults; models/cnn_backbone.py:151,158,246,351) -----------------------------
 * coef = scale | shift | mean | invstd (4*C floats).  finalize also updates running_mean/var (momentum, unbiased var)
 * and num_batches_tracked when those pointers are non-NULL. */
int vqa_bn_stats_finalize(const float* part, int tiles, int C, double count, const float* gamma, const float* beta,
                          float* running_mean, float* running_var, long long* num_batches_tracked, float momentum, float eps,
                          double* scratch /* >= 64*2*C */, float* coef, hipStream_t stream);
int vqa_bn_eval_coef(int C, const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                     float eps, float* coef, hipStream_t stream);
/* out = [relu](y*scale+shift [+ res | + res*rscale+rshift])   -- BN + residual add + ReLU (cnn_backbone.py:186-195) */
int vqa_bn_apply(int dtype, const void* y, const float* coef, const void* res, const float* rcoef, void* out,
                 long long numel, int C, int relu, hipStream_t stream);
/* the same for the LAST residual block of a stage, with the squeeze-excitation global-average-pool sums folded in: also writes the
   column sums of the stored values per (sample, row chunk) to part[B][vqa_bn_apply_pool_chunks()][C]; vqa_se_fwd(pool_part = part)
   folds them instead of re-reading the stage output (models/cnn_backbone.py:194-197 -> models/attention_modules.py:109-112) */
int vqa_bn_apply_pool_chunks(int dtype, int HW, int C);
int vqa_bn_apply_pool(int dtype, const void* y, const float* coef, const void* res, const float* rcoef, void* out, int B, int HW, int C,
                      int relu, float* part, hipStream_t stream);
/* Fixed-point statistics (round 3).  A producer launched with stats_mode = 1 (vqa_igemm, vqa_conv3x3_c64p) adds its per-workgroup
   fp32 partial sums  sum y | sum y^2  to acc[vqa_bn_acc_words(2, C)] (unsigned 64-bit, each sum split exactly into a 2^-4 plane and a 2^-50 plane, caller-zeroed; the flag
   word between the planes counts partials that were non-finite or beyond 2^41 -> NaN statistics; the total cannot wrap, csrc/common.h) with integer atomics: order-independent, hence bit-reproducible, and complete
   when the producer ends.  vqa_bn_apply_acc then does finalize (fp64, nn.BatchNorm2d training formulas, running-statistics update,
   coef_out [4][C] = scale | shift | mean | invstd for the backward) + apply (+ res | + BatchNorm(res) from racc, + ReLU) in ONE
   launch -- the finalize launches between conv and apply are gone.  pool_part != NULL: also the SE pooling sums (vqa_bn_apply_pool).
   Backward: vqa_bn_bwd_reduce(acc_mode = 1) / vqa_se_bwd(bn_acc_mode = 1) add  sum g | sum g*xhat | sum g*xhat2  (same format) to
   facc[vqa_bn_acc_words(3, C)]; vqa_bn_bwd_apply_acc derives the apply coefficients in its prologue and adds d gamma / d beta. */
int vqa_bn_acc_words(int K, int C);   /* 64-bit words of an accumulator for K sums x C channels: R = clamp(512/C, 1, 8) replicas
                                         (same-address atomics are serialised, ~21 ns each) + the flag word; K = 2 forward, 3 backward */
int vqa_bn_apply_acc(int dtype, const void* y, const unsigned long long* acc, const float* gamma, const float* beta, float* running_mean,
                     float* running_var, long long* num_batches_tracked, float* coef_out, const void* res,
                     const unsigned long long* racc, const float* rgamma, const float* rbeta, float* rrunning_mean, float* rrunning_var,
                     long long* rnum_batches_tracked, float* rcoef_out, void* out, int B, int HW, int C, int relu, double count,
                     float momentum, float eps, float* pool_part, hipStream_t stream);
int vqa_bn_bwd_blocks(long long rows);
int vqa_bn_bwd_reduce(int dtype, const void* dout, const void* outact, const void* y, const float* coef, const void* y2,
                      const float* coef2, float* slab /* [blocks][3][C], or the u64 accumulator [vqa_bn_acc_words(3, C)] (replicas x two planes + flag) when acc_mode = 1 */, long long rows,
                      int C, int self_mask /* mask = relu(bn(y))>0 from y */, int acc_mode, hipStream_t stream);
int vqa_bn_bwd_apply_acc(int dtype, const void* dout, const void* outact, const void* y, const unsigned long long* facc, const float* gamma,
                         const float* coef, float* dgamma, float* dbeta, void* dy, const void* y2, const float* gamma2, const float* coef2,
                         float* dgamma2, float* dbeta2, void* dy2, long long numel, int C, double count, int self_mask, hipStream_t stream);
int vqa_bn_bwd_finalize(const float* slab, int nblk, int C, int which, double count, const float* gamma, const float* coef,
                        int training, float* dgamma, float* dbeta, float* bcoef /* 3*C */, hipStream_t stream);
int vqa_bn_bwd_apply(int dtype, const void* dout, const void* outact, const void* y, const float* bcoef, void* dy,
                     const void* y2, const float* bcoef2, void* dy2, long long numel, int C, const float* mask_coef /* or NULL */,
                     hipStream_t stream);

/* ---- stem tail: BN + ReLU + MaxPool2d(3,2,1) fused (models/cnn_backbone.py:351-353) ----------------------------- */
int vqa_stem_pool_fwd(int dtype, const void* y, const float* coef, void* out, uint8_t* idx, int B, int H, int W, int C, hipStream_t stream);
int vqa_stem_bwd_apply(int dtype, const void* dpool, const uint8_t* idx, const void* y, const float* coef, const float* bcoef,
                       void* dy, int B, int H, int W, int C, hipStream_t stream);

/* ---- SEAttention.forward (models/attention_modules.py:109-136) and its backward ---------------------------------- */
/* C / (16 / sizeof element) must divide 256; the bottleneck 1 <= Cr <= C (any se_reduction), else VQA_EARG */
int vqa_se_fwd(int dtype, const void* x, const float* w1, const float* w2, float* pooled, float* hidden, float* scale,
               void* out, int B, int HW, int C, int Cr,
               const float* pool_part /* or NULL: pool x here */, int pool_chunks /* = vqa_bn_apply_pool_chunks */, hipStream_t stream);
/* bn_y / bn_coef / bn_slab (all or none): dx is the gradient entering the BatchNorm whose conv output is bn_y (the stage's last bn2);
   its backward column sums sum dx | sum dx*xhat(bn_y) are written to bn_slab[vqa_se_bwd_blocks()][3][C] (the layout
   vqa_bn_bwd_finalize reads) in the same pass, so the caller skips vqa_bn_bwd_reduce for that BatchNorm */
int vqa_se_bwd_blocks(int dtype, int B, int HW, int C);
long long vqa_se_bwd_scratch(int dtype, int B, int HW, int C, int Cr);   /* floats of `scratch` below */
/* bn_acc_mode 1: bn_slab is the u64 fixed-point accumulator (vqa_bn_acc_words(3, C)) instead of a float slab */
int vqa_se_bwd(int dtype, const void* dout, const void* x, const float* w1, const float* w2, const float* pooled,
               const float* hidden, const float* scale, float* scratch /* vqa_se_bwd_scratch() floats */, void* dx,
               float* dw1, float* dw2 /* both NULL: data gradient only, no weight-gradient launch */,
               int B, int HW, int C, int Cr, int mask_out /* dx *= (x > 0): x is a post-ReLU activation */,
               const void* bn_y, const float* bn_coef, float* bn_slab /* or the u64 accumulator when bn_acc_mode = 1 */, int bn_acc_mode,
               hipStream_t stream);
/* ---- SpatialAttention.forward (models/attention_modules.py:223-243) and its backward ----------------------------- */
/* C / (16 / sizeof element) must divide 256, else VQA_EARG before anything is written; the max ignores NaN (torch propagates it) */
int vqa_spatial_fwd(int dtype, const void* x, const float* w /* (1,2,7,7) */, float* pooled2, int* argmax, float* amap,
                    void* out, int B, int H, int W, int C, hipStream_t stream);
long long vqa_spatial_bwd_scratch(int B, int H, int W);   /* floats of `scratch` below (3*B*H*W + the conv-weight partial sums) */
int vqa_spatial_bwd(int dtype, const void* dout, const void* x, const float* w, const float* pooled2, const int* argmax,
                    const float* amap, float* scratch /* vqa_spatial_bwd_scratch() floats */, void* dx,
                    float* dw /* NULL: data gradient only */, int B, int H, int W, int C,
                    hipStream_t stream);
int vqa_nhwc_to_nchw(int dtype, const void* in, float* out, int B, int HW, int C, hipStream_t stream);   /* aux['image_features'] */
int vqa_nchw_to_nhwc(int dtype, const float* in, void* out, int B, int HW, int C, hipStream_t stream);

/* ---- token side ------------------------------------------------------------------------------------------------------
 * embedding*sqrt(d) + sinusoidal PE + dropout (models/text_encoder.py:504-510,112-114); padding_idx 0 gets no gradient */
int vqa_embed_fwd(int dtype, const long long* ids, const float* emb, const float* pe, void* out, int rows, int L, int D, int V,
                  float scale, float p, unsigned long long seed, hipStream_t stream);
int vqa_embed_bwd(int dtype, const long long* ids, const void* dout, float* demb, int rows, int D, int V, float scale, float p,
                  unsigned long long seed, hipStream_t stream);
/* nn.LayerNorm(eps 1e-5) (+dropout, + addrow[row % period]: ImageFeatureProjector, models/fusion.py:98-112) */
int vqa_layernorm_fwd(int dtype, const void* x, const float* gamma, const float* beta, void* out, float* mean_rstd, int rows, int D,
                      float eps, float p, unsigned long long seed, const float* addrow, int period, hipStream_t stream);
/* Fixed-order reductions.  The entries below that reduce over workgroups take `ws` (uninitialised float scratch, sized by the
 * matching *_ws query): every workgroup stores its partial sums to its own row and a second launch issued by the same entry
 * folds the rows in index order (bit-reproducible run to run).  With ws == NULL they fall back to float atomics (same value up
 * to rounding order). */
long long vqa_layernorm_bwd_ws(int dtype, int rows, int D, int period /* 0 when dadd == NULL */);
int vqa_layernorm_bwd(int dtype, const void* dout, const void* x, const float* gamma, const float* mean_rstd, const void* addend,
                      void* dx, float* dgamma, float* dbeta, int rows, int D, float p, unsigned long long seed, float* dadd,
                      int period, float* ws, int defer_fold /* 1: skip the fold launch(es), the caller runs vqa_fold_group later */,
                      hipStream_t stream);
/* folds of a deferred call: returns their number, 5 values per fold in out[10]: {ws offset (floats), rows, row stride, columns, n0};
   fold 0 -> (dgamma | dbeta) split at n0 = D, fold 1 (position-embedding sum) -> dadd */
int vqa_layernorm_bwd_folds(int dtype, int rows, int D, int period, long long* out);
/* softmax(QK^T/sqrt(hd) [keys with kmask==0 -> -inf]) (dropout) V, one wave per (batch, head)
 * (models/text_encoder.py:237-258, models/cross_attention.py:176-198); probs = softmax before dropout [B][H][Lq][Lk] */
int vqa_attention_fwd(int dtype, const void* q, const void* k, const void* v, int ldq, int ldk, int ldv, const float* kmask,
                      float* probs, void* ctx, int ldc, int B, int H, int Lq, int Lk, int hd, float p, unsigned long long seed,
                      hipStream_t stream);
/* bf16 MFMA variant (Lq <= 32, Lk <= 64, hd 32|64): QK^T and PV as v_mfma_f32_32x32x16_bf16 tiles, softmax in registers */
int vqa_attention_fwd_mfma(const void* q, const void* k, const void* v, int ldq, int ldk, int ldv, const float* kmask, float* probs,
                           void* ctx, int ldc, int B, int H, int Lq, int Lk, int hd, float p, unsigned long long seed, hipStream_t stream);
/* cross-attention forward whose K / V rows (and kmask rows) for query batch b are those of image kv_index[b] (many questions per
 * image from one cached image encoding): k, v hold n_kv images of Lk rows each; probs / ctx are per query batch as in
 * vqa_attention_fwd(_mfma).  Inference only: no dropout.  A query batch whose index lies outside [0, n_kv) loads nothing and gets
 * NaN in its probs and ctx rows.  The _mfma form has the limits of vqa_attention_fwd_mfma and takes no dtype (bf16).
 * kmask (may be NULL) masks with -inf like every attention entry here, so an image whose keys are ALL masked gives NaN rows; the
 * modelled cross-attention fills with -1e9 instead, which gives a uniform row there and the same zeros for a partly masked row.
 * The engine passes no key mask to cross-attention, so the difference cannot be reached from the model. */
int vqa_attention_fwd_idx(int dtype, const void* q, const void* k, const void* v, int ldq, int ldk, int ldv, const int* kv_index,
                          int n_kv, const float* kmask, float* probs, void* ctx, int ldc, int B, int H, int Lq, int Lk, int hd,
                          hipStream_t stream);
int vqa_attention_fwd_mfma_idx(const void* q, const void* k, const void* v, int ldq, int ldk, int ldv, const int* kv_index, int n_kv,
                               const float* kmask, float* probs, void* ctx, int ldc, int B, int H, int Lq, int Lk, int hd,
                               hipStream_t stream);
/* Backward of vqa_attention_fwd from the saved probs (the dropout mask is regenerated from p and seed): dq [B*Lq], dk, dv [B*Lk].
 * A probs row that is NaN (every key masked) gives NaN in that batch's dq, dk and dv.  Its tiles need about twice the forward's LDS
 * (the 160 KiB limit is met at a smaller Lk), so there are shapes the forward accepts and this entry refuses (status 1000, nothing
 * written): at Lq 20, hd 64 the forward takes Lk <= 264, the backward Lk <= 225. */
int vqa_attention_bwd(int dtype, const void* dctx, int ldc, const void* q, const void* k, const void* v, int ldq, int ldk, int ldv,
                      const float* probs, void* dq, void* dk, void* dv, int lddq, int lddk, int lddv, int B, int H, int Lq, int Lk,
                      int hd, float p, unsigned long long seed, hipStream_t stream);
/* bf16 MFMA form of vqa_attention_bwd (Lq <= 32, Lk <= 64, hd in {32, 64}, row strides multiples of 8); same arguments minus dtype */
int vqa_attention_bwd_mfma(const void* dctx, int ldc, const void* q, const void* k, const void* v, int ldq, int ldk, int ldv,
                           const float* probs, void* dq, void* dk, void* dv, int lddq, int lddk, int lddv, int B, int H, int Lq, int Lk,
                           int hd, float p, unsigned long long seed, hipStream_t stream);
/* attention backward with an upstream gradient on the saved softmax (graph-connected aux['cross_attention_weights']):
 * dprobs [B][H][Lq][Lk] fp32 like probs; dP = keep_scale * (dctx V^T) + dprobs, dS = P * (dP - rowsum(P * dP)) / sqrt(hd), dV unchanged.
 * Same arguments as vqa_attention_bwd / vqa_attention_bwd_mfma plus dprobs (never NULL); with dprobs == 0 the results are bit-equal. */
int vqa_attention_bwd_dp(int dtype, const void* dctx, int ldc, const void* q, const void* k, const void* v, int ldq, int ldk, int ldv,
                         const float* probs, const float* dprobs, void* dq, void* dk, void* dv, int lddq, int lddk, int lddv, int B, int H,
                         int Lq, int Lk, int hd, float p, unsigned long long seed, hipStream_t stream);
int vqa_attention_bwd_mfma_dp(const void* dctx, int ldc, const void* q, const void* k, const void* v, int ldq, int ldk, int ldv,
                              const float* probs, const float* dprobs, void* dq, void* dk, void* dv, int lddq, int lddk, int lddv, int B, int H,
                              int Lq, int Lk, int hd, float p, unsigned long long seed, hipStream_t stream);
/* Many questions per image in training (VQAModel.forward_grouped, HipTrainer.step(image_index=)).
 * vqa_index_csr: the questions of each image in ascending question order -- offsets [U+1], order [N] (image u's questions are
 * order[offsets[u] .. offsets[u+1])).  Deterministic counting sort in one launch (U <= 32768), no host sync.  An index outside
 * [0, U) writes -1 to every offsets and order entry (the backward kernels below then write NaN, never a wrong sum). */
int vqa_index_csr(const int* kv_index, int N, int U, int* offsets, int* order, hipStream_t stream);
/* vqa_attention_fwd(_mfma)_idx with dropout (p, seed): the mask of (question b, head, i, j) is the one vqa_attention_fwd(_mfma)
 * draws for batch b, so an identity index is bit-equal to them. */
int vqa_attention_fwd_idx_train(int dtype, const void* q, const void* k, const void* v, int ldq, int ldk, int ldv, const int* kv_index,
                                int n_kv, const float* kmask, float* probs, void* ctx, int ldc, int B, int H, int Lq, int Lk, int hd,
                                float p, unsigned long long seed, hipStream_t stream);
int vqa_attention_fwd_mfma_idx_train(const void* q, const void* k, const void* v, int ldq, int ldk, int ldv, const int* kv_index, int n_kv,
                                     const float* kmask, float* probs, void* ctx, int ldc, int B, int H, int Lq, int Lk, int hd, float p,
                                     unsigned long long seed, hipStream_t stream);
/* Backward of the _idx_train forwards: dq [B*Lq] per question, dk / dv [n_kv*Lk] per IMAGE = the sum over the image's questions
 * (offsets / order of vqa_index_csr over the same index), accumulated in fp32 in CSR order and rounded once; no float atomics.
 * One question per image: bit-equal to vqa_attention_bwd(_mfma).  An image without questions gets zeros.  The generic form needs
 * Lk * hd <= 10240 besides the LDS limit of vqa_attention_bwd; the _mfma form has the limits of vqa_attention_bwd_mfma. */
int vqa_attention_bwd_idx(int dtype, const void* dctx, int ldc, const void* q, const void* k, const void* v, int ldq, int ldk, int ldv,
                          const float* probs, const int* offsets, const int* order, int n_kv, void* dq, void* dk, void* dv,
                          int lddq, int lddk, int lddv, int B, int H, int Lq, int Lk, int hd, float p, unsigned long long seed,
                          hipStream_t stream);
int vqa_attention_bwd_mfma_idx(const void* dctx, int ldc, const void* q, const void* k, const void* v, int ldq, int ldk, int ldv,
                               const float* probs, const int* offsets, const int* order, int n_kv, void* dq, void* dk, void* dv,
                               int lddq, int lddk, int lddv, int B, int H, int Lq, int Lk, int hd, float p, unsigned long long seed,
                               hipStream_t stream);
/* Device-side accuracy counters: counters[3] (u64) += {top-1 correct, top-5 correct, samples} for fp32 logits [B][N] and i64 targets.
 * Replaces the argmax/topk + .cpu() + .item() of VQAAccuracy.update (utils/metrics.py:55-94); ties resolve to the lowest index. */
int vqa_accuracy_update(const float* logits, const long long* targets, unsigned long long* counters, int B, int N, hipStream_t stream);
/* Top-k answers with their softmax probabilities in one launch (VQAModel.predict's softmax + topk; api/inference.py:228-246).
 * logits: fp32 or bf16 [B][ld], ld >= N.  allowed: optional 0/1 bytes, allowed_ld == 0: one row [N] shared by every logits row, else
 * [B][allowed_ld] with allowed_ld >= N.  y[j] = logits[j] where allowed (or without a mask), else -inf.
 * Order: a before b when y[a] > y[b], or y[a] == y[b] and a < b; NaN ranks above every number, NaNs among themselves by index
 *   (torch.sort(y, descending=True, stable=True)); decided on y itself, so idx [B][K] (i64) is exact.
 * probs [B][K] (fp32) = exp(scale * y[idx] - m) / sum_j exp(scale * y[j] - m), m = max_j scale * y[j], scale = 1 / temperature:
 *   softmax(y * scale) gathered at idx, IEEE arithmetic on special rows (a row holding a NaN, or with nothing allowed, gives NaN for all
 *   K); scale == 1 changes no bit.  logits_f (optional, fp32 [B][N]) receives the RAW logits (not the masked ones).
 * No atomics, no scratch; bit-reproducible.  Status 1000 without a launch: NULL logits / idx / probs; B, N or K < 1; K > 64; K > N;
 * ld < N; allowed_ld neither 0 nor >= N; scale not finite or <= 0; dtype other than 0 (fp32) / 1 (bf16). */
int vqa_softmax_topk(int dtype, const void* logits, long long ld, const unsigned char* allowed, long long allowed_ld, float scale,
                     long long* idx, float* probs, float* logits_f, int B, int N, int K, hipStream_t stream);
/* Soft answer scores (VQA v2, ten annotator answers per question; utils/metrics.py:12-19 acc(ans) = min(1, #agreeing annotators / 3)).
 * vqa_answer_scores: answers [B][A] (i64 answer ids, -1 = not in the vocabulary, A <= 64) -> per row the distinct in-vocabulary ids in
 *   order of first occurrence (ids), their number of occurrences (counts) and weights = min(1, count / 3) in fp32 (mode 0) or that
 *   divided by the row's sum taken in slot order (mode 1; a row without an in-vocabulary answer stays zero).  Unused slots: -1 / 0 / 0.
 *   An id < -1 or >= N: *err (may be NULL) += 1 per such row, the row becomes {N, -1, ...} / 0 / 0 so that the loss rejects it.
 * vqa_cross_entropy_soft: vqa_cross_entropy with t[b][c] = sum of weights[b][k] over ids[b][k] == c (duplicates add up, -1 slots are
 *   skipped), W[b] = sum_c t[b][c]:  loss += sum_b (W[b] * lse[b] - sum_k w[b][k] * x[b][ids[b][k]]) / B  (F.cross_entropy with
 *   probability targets), dlogits = (W * softmax - t) * gscale / B (may be NULL).  An id < -1 or >= N is a bad target as there.
 *   K = 1 with weight 1 gives the bits of vqa_cross_entropy.  counts + acc (both optional; acc without counts is an argument error):
 *   acc[0] += min(3, votes for the row's arg-max) (integer thirds of the challenge accuracy), acc[1] += 1, per row, in the same pass.
 * vqa_challenge_accuracy_update: those two counters alone, from fp32 logits (utils/metrics.py:136-184 VQAChallengeAccuracy without
 *   the string comparison on the host); ties resolve to the lowest index. */
int vqa_answer_scores(const long long* answers, int* ids, float* weights, int* counts, int B, int A, int N, int mode, int* err,
                      hipStream_t stream);
int vqa_cross_entropy_soft(int dtype, const void* logits, const int* ids, const float* weights, int K, float* loss, void* dlogits,
                           float* logits_f32, int B, int N, float gscale, int* err, float* ws, const int* counts,
                           unsigned long long* acc, hipStream_t stream);
int vqa_challenge_accuracy_update(const float* logits, const int* ids, const int* counts, int K, unsigned long long* acc, int B, int N,
                                  hipStream_t stream);
/* Sigmoid + binary cross-entropy against the soft answer scores (the VQA v2 recipe): vqa_cross_entropy_soft's arguments and the same
 * t[b][c] = sum of weights[b][k] over ids[b][k] == c (duplicates add up, -1 slots are skipped, nothing is clamped).
 *   loss += (1/B) * sum_b sum_c [ max(x,0) + log1p(exp(-|x|)) - x*t ]  = F.binary_cross_entropy_with_logits(x, t, reduction="sum") / B:
 *   summed over answers, averaged over questions; the stable form (x = +-90 gives finite values); the x*t part is taken from the K
 *   slots in slot order.  dlogits = (sigmoid(x) - t) * gscale / B in the compute dtype (may be NULL: the loss alone).
 *   A row without an in-vocabulary answer (t all zero) is NOT a zero row here: it gets sigmoid(x) * gscale / B, every logit is pushed
 *   down.  Under vqa_cross_entropy_soft that row is a zero row; the difference is intended.
 *   logits_f32 (optional) receives the raw logits, bit for bit.  An id < -1 or >= N is never read: the row adds NaN to the loss, gets
 *   a NaN gradient row and counts one in *err (may be NULL), as in vqa_cross_entropy_soft.
 *   ws (B floats, or NULL): per-row terms go to ws and are folded in row order -- no float atomic on *loss, two launches give the same
 *   bits; NULL: float atomics on *loss.  counts + acc (both optional): the challenge accuracy in integer thirds in the same pass,
 *   acc[0] += min(3, votes for the row's arg-max), acc[1] += 1; the arg-max is the lowest index that holds the row maximum.
 * Status 1000 without a launch: NULL logits / ids / weights; K < 1 or K > 64; B < 1 or N < 1; acc without counts; dtype other than
 * 0 (fp32) / 1 (bf16); gscale not finite. */
int vqa_bce_soft(int dtype, const void* logits, const int* ids, const float* weights, int K, float* loss, void* dlogits,
                 float* logits_f32, int B, int N, float gscale, int* err, float* ws, const int* counts, unsigned long long* acc,
                 hipStream_t stream);
/* masked mean over tokens (models/fusion.py:303-313, models/text_encoder.py:522-527) */
/* both masked means of the fusion tail in one launch (round 4): out[B][2D] = [mean_m(x0) | mean_m(x1)] with the same mask, and the
 * matching backward dx{0,1}[b][l][:] = dcat[b][{0,D}:] * m[b][l] / cnt (models/fusion.py:281-296); per-element arithmetic of
 * vqa_masked_pool_fwd / _bwd (bit-equal). */
int vqa_masked_pool_pair_fwd(int dtype, const void* x0, const void* x1, const float* mask, void* out, int B, int L, int D, hipStream_t stream);
int vqa_masked_pool_pair_bwd(int dtype, const void* dcat, const float* mask, void* dx0, void* dx1, int B, int L, int D, hipStream_t stream);
int vqa_masked_pool_fwd(int dtype, const void* x, const float* mask, void* out, int ldo, int col0, int B, int L, int D, hipStream_t stream);
int vqa_masked_pool_bwd(int dtype, const void* dpool, int ldo, int col0, const float* mask, const void* addend, void* dx,
                        int B, int L, int D, hipStream_t stream);
/* GatingMechanism.forward (models/fusion.py:160-166): fused = g*att + (1-g)*txt, g = sigmoid(z), cat = [att|txt] */
int vqa_gate_fwd(int dtype, const void* z, const void* cat, void* fused, int B, int D, hipStream_t stream);
int vqa_gate_bwd(int dtype, const void* dfused, const void* z, const void* cat, void* dz, void* dcat, int B, int D, hipStream_t stream);
int vqa_add(int dtype, const void* a, const void* b, void* out, long long n, hipStream_t stream);
/* gradient tap: acc (compute dtype) += g (fp32).  layout 0: acc[r*ld + c] += g[r*cols + c] (r < rows, c < cols, ld >= cols);
 * layout 1 (NCHW -> NHWC): acc is [rows][cols] with rows = B*HW and ld = HW, g is [B][cols][HW] (aux['image_features']) */
int vqa_grad_tap_add(int dtype, const float* g, void* acc, int rows, int cols, int ld, int layout, hipStream_t stream);
/* gradient at the pre-activation of linear(+bias)(+ReLU)(+dropout); dbias += column sums */
long long vqa_bias_act_bwd_ws(int dtype, int M, int N);
int vqa_bias_act_bwd(int dtype, const void* dout, const void* outact, void* dz, float* dbias, int M, int N, float p,
                     unsigned long long seed, float* ws, int defer_fold, hipStream_t stream);
int vqa_bias_act_bwd_fold_rows(int dtype, int M, int N);   /* deferred fold: {offset 0, this many rows, stride N, N columns, n0 = N} -> dbias */
/* the deferred folds of any number of calls in one launch per 48 jobs: dst0_j[c] (c < n0_j) / dst1_j[c - n0_j] += sum_r part_j[r*stride_j + c] */
int vqa_fold_group(int njobs, const float* const* part, const int* nrows, const long long* stride, const int* ncols, float* const* dst0,
                   const int* n0, float* const* dst1, hipStream_t stream);
/* nn.CrossEntropyLoss() mean (training/train.py:120): loss += mean NLL, dlogits = (softmax-onehot)*gscale/B.
   err (device int, may be NULL): += number of rows whose target is outside [0, N) -- the reference raises there; such rows are
   never read out of bounds, they add NaN to the loss and get a NaN gradient row. */
int vqa_cross_entropy(int dtype, const void* logits, const long long* targets, float* loss, void* dlogits, float* logits_f32,
                      int B, int N, float gscale, int* err, float* ws /* B floats, or NULL: float atomics on *loss */, hipStream_t stream);
/* nn.CrossEntropyLoss(weight=, ignore_index=, label_smoothing=) mean: vqa_cross_entropy's arguments, then the options.
 * class_weight [N] fp32 (NULL: all ones); has_ignore 0: no target is ignored; label_smoothing eps in [0, 1].
 * keep[b] = target b != ignore_index (also when ignore_index lies in [0, N)), wy[b] = keep[b] * w[t_b], W = sum_b wy[b], Sw = sum_c w[c]:
 *   loss    += [ (1-eps) * sum_b wy[b] * (-lp[b][t_b]) + eps/N * sum_b keep[b] * sum_c w[c] * (-lp[b][c]) ] / W       (lp = log_softmax)
 *   dlogits  = [ (1-eps) * wy[b] * (p[b][c] - [c == t_b]) + eps/N * keep[b] * (Sw * p[b][c] - w[c]) ] * gscale / W    (may be NULL)
 * = F.cross_entropy(logits, target, weight, ignore_index=, label_smoothing=, reduction="mean").  An ignored row adds no loss term,
 * gets a zero gradient row and is never counted in *err; any other target outside [0, N) is a bad target as in vqa_cross_entropy
 * (it counts in W with weight 1).  W == 0 (all rows ignored, or all kept rows of weight 0): the loss is NaN as in torch, dlogits
 * is all ZERO (torch: zero without weights, NaN with weights -- this entry deviates on purpose) and *empty (may be NULL) += 1.
 * acc (may be NULL): VQAAccuracy's {correct, correct_top5, total} += over the kept rows in the same pass, vqa_accuracy_update's
 * rank rule (lowest index wins ties), a bad target counts in total as wrong.  W and Sw are summed by every wave in one fixed order:
 * with ws (B floats) there is no float atomic and two launches give the same bits.  With class_weight NULL, eps 0 and no ignored
 * target every output has the bits of vqa_cross_entropy.  Status 1000 without a launch: NULL logits / targets, B or N < 1, dtype
 * not 0 / 1, label_smoothing outside [0, 1] or NaN, gscale not finite. */
int vqa_cross_entropy_opts(int dtype, const void* logits, const long long* targets, float* loss, void* dlogits, float* logits_f32,
                           int B, int N, float gscale, int* err, float* ws, const float* class_weight, long long ignore_index,
                           int has_ignore, float label_smoothing, unsigned long long* acc, int* empty, hipStream_t stream);
int vqa_convert(int dtype_in, int dtype_out, const void* src, void* dst, long long n, hipStream_t stream);
/* clip_grad_norm_(max_norm) + AdamW over flat fp32 buffers (training/train.py:204-208,127-132).
   skip (device int, may be NULL): when skip[0] != 0 the launch changes NOTHING (parameters, moments) and adds skip[0] to
   skipped[0], 1 to skipped[1] and 1 to skipped[2] (device int[3], may be NULL; [0] / [1] are the caller's to reset, [2] never) -- a
   step whose CrossEntropy saw an out-of-range target raises in the reference before optimizer.step(), so the model must survive it.
   calls: how many times the caller has launched vqa_adamw on this state, this launch included (>= 1).  Adam's step number
   t = calls - skipped[2] is formed ON THE DEVICE (bias corrections 1 - beta^t in double, like torch.optim.AdamW), so a skipped launch
   never advances it, whatever the host knows. */
int vqa_sumsq(const float* g, long long n, float* out /* >= 2049 floats: [0] result (bit-reproducible), rest scratch */, hipStream_t stream);
int vqa_adamw(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2, float eps,
              float weight_decay, long long calls, const float* sumsq, float max_norm, float gscale,
              const int* skip, int* skipped,
              void* p_bf16 /* or NULL: also write the bf16 copy of the updated parameters (the operand buffer of the next forward) */,
              hipStream_t stream);

/* The same over a device table of TRAINABLE ranges (fine-tuning with frozen parameters): elements outside them are never read or
   written (parameters, moments and the bf16 copy stay put).  table: R <= 512 int64 rows (R = 0 with n = 0: nothing trains) {lo, hi, pos, lag index}: [lo, hi) of the flat
   buffer, pos = its start in the concatenation of the ranges (ascending, pos[0] = 0); lo, hi, pos multiples of 4; n = total trainable
   elements.  The norm folds in a fixed order.  Adam's step number of a range is calls - skipped[2] - lag[its lag index]: lag[j] (device
   int per parameter) counts applied steps during which parameter j was frozen -- after an applied launch lag[frozen[k]] += 1 for the nf
   frozen parameters listed, as torch.optim.AdamW advances a parameter's step only while it has a gradient. */
int vqa_sumsq_ranges(const float* g, const long long* table, int R, long long n, float* out /* >= 2049 floats, as vqa_sumsq */,
                     hipStream_t stream);
int vqa_adamw_ranges(float* p, const float* g, float* m, float* v, const long long* table, int R, long long n, float lr, float beta1,
                     float beta2, float eps, float weight_decay, long long calls, const float* sumsq, float max_norm, float gscale,
                     const int* skip, int* skipped, int* lag, const int* frozen, int nf, void* p_bf16, hipStream_t stream);

/* Exponential moving average of the weights, kept by the optimizer launch itself.
   vqa_adamw_ema = vqa_adamw (p, m, v and the bf16 copy get the same bits) and, for every element it updated,
       ema[i] = d * ema[i] + (1 - d) * p_new[i]          (fp32: 1 - d and (1 - d) * p_new rounded once each, then one fma)
   from the p_new still in a register: the average costs one read and one write of `ema`, no launch and no second read of p.
   d = ema_decay when ema_warmup == 0, else min(ema_decay, (1 + t) / (10 + t)) in fp32 with Adam's step number t = calls - skipped[2]
   formed on the device.  A skipped launch (skip[0] != 0) leaves `ema` untouched bit for bit and advances no warm-up.
   vqa_adamw_ranges_ema = vqa_adamw_ranges with the same addition: `ema` is neither read nor written outside the trainable ranges,
   and the warm-up of a range uses that range's OWN step number calls - skipped[2] - lag[its lag index] -- the average of a parameter
   advances only while the parameter trains, exactly as its Adam step does (a part thawed late starts its warm-up when it thaws).
   vqa_ema_update: the same update as a pass of its own over a flat buffer, ema[i] = d * ema[i] + (1 - d) * p[i] with the EFFECTIVE d
   given by the caller (torch.optim loops); the same p and ema give the bits the fused launches give.  Any alignment (16-byte
   accesses when both pointers allow them).
   Status 1000 without a launch: ema NULL (vqa_ema_update: or p), ema_decay / d outside [0, 1] or NaN, n < 0, and whatever the entry
   they extend refuses. */
int vqa_adamw_ema(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2, float eps,
                  float weight_decay, long long calls, const float* sumsq, float max_norm, float gscale,
                  const int* skip, int* skipped, void* p_bf16, float* ema, float ema_decay, int ema_warmup, hipStream_t stream);
int vqa_adamw_ranges_ema(float* p, const float* g, float* m, float* v, const long long* table, int R, long long n, float lr, float beta1,
                         float beta2, float eps, float weight_decay, long long calls, const float* sumsq, float max_norm, float gscale,
                         const int* skip, int* skipped, int* lag, const int* frozen, int nf, void* p_bf16,
                         float* ema, float ema_decay, int ema_warmup, hipStream_t stream);
int vqa_ema_update(float* ema, const float* p, long long n, float d, hipStream_t stream);

/* ---- step state on the device (HipTrainer.step_graphed: the train step replayed from a captured HIP graph) ---------------------
   A captured launch freezes every by-value argument at its capture-time value.  What changes from step to step therefore lives in
   one device block, written by vqa_step_state_set -- a one-thread kernel, launched eagerly right before a replay; its arguments are
   copied at launch, so there is no staging buffer, no host-to-device copy and no host synchronisation -- and read by:
     * vqa_adamw_dev / vqa_adamw_ema_dev / vqa_adamw_ranges_dev / vqa_adamw_ranges_ema_dev: the four entries above with lr, beta1, beta2,
       eps, weight_decay, calls, max_norm, gscale (and ema_decay, ema_warmup) taken from the block instead of by value; the kernels load
       the block into locals and run the by-value kernels' body, so p, m, v, the bf16 copy, ema and skipped get the same bits.  The
       range checks the by-value entries make on calls and ema_decay are the caller's (the host cannot see the block);
     * every kernel that takes a dropout seed.  A seed word is self-describing: with bit 63 clear it is the seed itself, as before
       (rank << 44 | step << 12 | site never reaches bit 63); with bit 63 set, bits 0-47 are the device address of
       vqa_step_state::seed_step and bits 48-59 the site (< 4096), and the kernel uses *address | site.  seed_step holds
       rank << 44 | (step & 0xFFFFFFFF) << 12 of the step being run.  No signature changes: `unsigned long long seed` carries either form. */
typedef struct __attribute__((aligned(16))) vqa_step_state {
  long long calls;
  unsigned long long seed_step;
  float lr, b1, b2, eps, wd, max_norm, gscale, ema_decay;
  int ema_warmup;
} vqa_step_state;
int vqa_step_state_set(vqa_step_state* state, long long calls, unsigned long long seed_step, float lr, float beta1, float beta2, float eps,
                       float weight_decay, float max_norm, float gscale, float ema_decay, int ema_warmup, hipStream_t stream);
int vqa_adamw_dev(float* p, const float* g, float* m, float* v, long long n, const vqa_step_state* state, const float* sumsq,
                  const int* skip, int* skipped, void* p_bf16, hipStream_t stream);
int vqa_adamw_ema_dev(float* p, const float* g, float* m, float* v, long long n, const vqa_step_state* state, const float* sumsq,
                      const int* skip, int* skipped, void* p_bf16, float* ema, hipStream_t stream);
int vqa_adamw_ranges_dev(float* p, const float* g, float* m, float* v, const long long* table, int R, long long n,
                         const vqa_step_state* state, const float* sumsq, const int* skip, int* skipped, int* lag, const int* frozen, int nf,
                         void* p_bf16, hipStream_t stream);
int vqa_adamw_ranges_ema_dev(float* p, const float* g, float* m, float* v, const long long* table, int R, long long n,
                             const vqa_step_state* state, const float* sumsq, const int* skip, int* skipped, int* lag, const int* frozen,
                             int nf, void* p_bf16, float* ema, hipStream_t stream);

/* ---- parameter groups (HipTrainer(param_groups=...)): a learning-rate scale and a weight decay per group of parameters ----------
   Every range of the table belongs to one of at most 16 groups: group_of_range is a device int32 array of R entries in 0 ... 15 (the
   caller's to keep there; the kernels take an entry modulo 16, so none reads outside the block).  A range of group g is updated as
   vqa_adamw_ranges updates it, with  lr * groups->lr_scale[g]  in the place of lr and  groups->wd[g]  in the place of weight_decay
   (the launch's own weight_decay is not used): torch.optim.AdamW with one param group per group.  The norm and its clip stay global
   (vqa_sumsq_ranges over the same table).  lr_scale[g] == 0 is not freezing: both moments, the step number and the average advance,
   the parameter keeps its value and the bf16 copy is written from it.  With every lr_scale 1 and every wd the launch's weight_decay
   the four entries give the bits of the vqa_adamw_ranges entries they extend: they are the same kernel body.
   The block lives on the device and is read there when a kernel runs -- by the by-value entries and the _dev entries alike, so an
   eager and a captured step share one mechanism.  vqa_group_hyper_set writes it with a one-thread kernel: lr_scale and wd are HOST
   arrays of G entries, read at call time and handed to the kernel by value (no staging buffer, no copy, no host synchronisation);
   entries G ... 15 of the block are set to 0.  wd is the effective value per group.
   Status 1000 without a launch: vqa_group_hyper_set -- G outside 1 ... 16, a NULL or not 16-byte-aligned block, a NULL array, a value
   that is negative or not finite; the four entries -- a NULL group_of_range, a NULL or misaligned groups, and whatever the
   vqa_adamw_ranges entry they extend refuses. */
#define VQA_GROUPS_MAX 16
typedef struct __attribute__((aligned(16))) vqa_group_hyper {
  float lr_scale[VQA_GROUPS_MAX];
  float wd[VQA_GROUPS_MAX];
} vqa_group_hyper;
int vqa_group_hyper_set(vqa_group_hyper* block, int G, const float* lr_scale, const float* wd, hipStream_t stream);
int vqa_adamw_groups(float* p, const float* g, float* m, float* v, const long long* table, int R, long long n, float lr, float beta1,
                     float beta2, float eps, float weight_decay, long long calls, const float* sumsq, float max_norm, float gscale,
                     const int* skip, int* skipped, int* lag, const int* frozen, int nf, void* p_bf16, const int* group_of_range,
                     const vqa_group_hyper* groups, hipStream_t stream);
int vqa_adamw_groups_ema(float* p, const float* g, float* m, float* v, const long long* table, int R, long long n, float lr, float beta1,
                         float beta2, float eps, float weight_decay, long long calls, const float* sumsq, float max_norm, float gscale,
                         const int* skip, int* skipped, int* lag, const int* frozen, int nf, void* p_bf16,
                         float* ema, float ema_decay, int ema_warmup, const int* group_of_range, const vqa_group_hyper* groups,
                         hipStream_t stream);
int vqa_adamw_groups_dev(float* p, const float* g, float* m, float* v, const long long* table, int R, long long n,
                         const vqa_step_state* state, const float* sumsq, const int* skip, int* skipped, int* lag, const int* frozen, int nf,
                         void* p_bf16, const int* group_of_range, const vqa_group_hyper* groups, hipStream_t stream);
int vqa_adamw_groups_ema_dev(float* p, const float* g, float* m, float* v, const long long* table, int R, long long n,
                             const vqa_step_state* state, const float* sumsq, const int* skip, int* skipped, int* lag, const int* frozen,
                             int nf, void* p_bf16, float* ema, const int* group_of_range, const vqa_group_hyper* groups,
                             hipStream_t stream);

/* ---- the non-finite guard (HipTrainer(nonfinite="skip" | "raise")): a step whose gradient is not finite never happened ----------
   vqa_sumsq_guard / vqa_sumsq_ranges_guard: vqa_sumsq / vqa_sumsq_ranges -- the same partial kernels, grids and fold order, so out[]
   holds the same bits -- whose ONE folding block also judges the step and writes the EFFECTIVE skip word, the word every vqa_adamw*
   entry takes as `skip` (and the lag update behind the range entries honours):
     bad_step (device int, may be NULL): rows of this step with an out-of-range target.  != 0: word[0] = bad_step[0], bad[0] += it,
       bad[1] += 1 (device int[2], may be NULL; the caller's to reset); the step stays a bad-target step and `nonfinite` rests;
     else out[0] NaN or +-inf (a NaN or inf element, or finite elements whose squares overflow the sum, as torch's norm would be inf):
       word[0] = 1, nonfinite[0] += 1 (the caller's to reset), nonfinite[1] += 1 (never reset);
     else word[0] = 0 and no counter is written.
   The AdamW launch behind it is given `word` as skip and a counter array of its own as skipped (skipped[2] = launches that did not
   count as a step, for whichever reason: Adam's step number stays calls - skipped[2]).  No launch is added to a step.
   vqa_buffers_save / vqa_buffers_restore: the BatchNorm running buffers, which the forward overwrites before the verdict exists.
   table: `rows` (1 ... 65535) int64 rows {device address (4-byte aligned), size in 32-bit words, word offset into scratch}; save copies
   every buffer into scratch (ahead of the forward), restore copies them back when word[0] != 0 and does nothing otherwise (behind
   the guarded norm).  Stable addresses: both can be captured.  The table is trusted as written.
   vqa_nonfinite_scan: counts[j] += non-finite elements of g[lo_j, hi_j) for the P (1 ... 2^20) int64 rows {lo, hi} of table (integer
   atomics: exact in any order; what lies between the rows -- the layout's alignment padding -- is not read).  The caller zeroes counts.
   Status 1000 without a launch: a NULL g / out / word / nonfinite / table / scratch / counts, n < 0, rows or P out of range, and what
   vqa_sumsq_ranges refuses. */
int vqa_sumsq_guard(const float* g, long long n, float* out /* as vqa_sumsq */, const int* bad_step, int* word, int* bad, int* nonfinite,
                    hipStream_t stream);
int vqa_sumsq_ranges_guard(const float* g, const long long* table, int R, long long n, float* out, const int* bad_step, int* word,
                           int* bad, int* nonfinite, hipStream_t stream);
int vqa_buffers_save(const long long* table, int rows, void* scratch, hipStream_t stream);
int vqa_buffers_restore(const long long* table, int rows, void* scratch, const int* word, hipStream_t stream);
int vqa_nonfinite_scan(const float* g, const long long* table, int P, int* counts, hipStream_t stream);

/* Row gather for cached image features (VQAModel.encode_features, ImageFeatures.select): dst[i] = src[index[i]] for i < n, rows of
   row_bytes bytes of any element type.  src holds n_src rows; index is device int32 [n] with every entry in [0, n_src) -- the caller
   checks the range; an entry outside it leaves its destination row unwritten and reads nothing.  16-byte vector loads and stores, one
   workgroup per 16 KB chunk of a row.  Status 1000 without a launch: row_bytes <= 0 or no multiple of 16, n or n_src negative, and
   for n > 0 a NULL or not 16-byte-aligned src / dst, a NULL index, n_src == 0, or 2^24 or more chunks (n * ceil(row_bytes / 16384)).  n == 0 launches nothing. */
int vqa_gather_rows(const void* src, const int* index, void* dst, int n, long long row_bytes, int n_src, hipStream_t stream);

/* Batch draw from a resident uint8 image bank (csrc/bank_ops.hip; dropin/data/image_bank.py ImageBank.batch): the random suffix of the
   training transform -- RandomCrop + RandomHorizontalFlip, data/preprocess.py:71-73 -- on images whose Resize was stored once.
   bank uint8 [n_rows][S][S][3] and out uint8 [B][O][O][3], both 16-byte aligned; rows device int32 [B]; crop_yx device int32 [B][2]
   as (y, x) or NULL (every origin (0, 0)); flip device uint8 [B] or NULL (no flip):
     out[b][y][x][c] = bank[rows[b]][cy_b + y][cx_b + (flip_b ? O-1-x : x)][c]
   Bytes are copied, never computed on.  Every per-sample argument is a device array, so one launch serves any B and the call can be
   captured; no scratch.  Offsets into the bank are 64-bit (21 846 rows of 256 x 256 x 3 pass 2^32 bytes); no byte outside
   [bank, bank + n_rows*S*S*3) is read -- a source row starts at cx*3, any alignment: the aligned dwords holding the wanted bytes are
   loaded and shifted -- and none outside out is written.
   A sample whose row is outside [0, n_rows) or whose origin is outside [0, S-O] in either axis keeps its out bytes as they were, reads
   nothing and adds 1 to *err (device int, may be NULL; the caller zeroes it).
   Status 1000 without a launch: n_rows < 1, B < 0, S or O below 4 or no multiple of 4 (output rows are whole dwords, as
   vqa_image_normalize's W % 4 == 0), O > S, S > 32768 (offsets inside one image are 32-bit), and for B > 0 a NULL or not
   16-byte-aligned bank / out or a NULL rows.  B == 0 launches nothing. */
int vqa_bank_batch(const uint8_t* bank, long long n_rows, int S, const int* rows, const int* crop_yx, const uint8_t* flip,
                   uint8_t* out, int B, int O, int* err, hipStream_t stream);

/* Per-tensor statistics of a flat fp32 buffer (csrc/stats_ops.hip; kernels.tensor_stats, HipTrainer(monitor=...)): a deterministic
   segmented reduction, one result row per table row, two launches, no float atomics, no host sync.
   table: device int64 [P][3] rows {lo, hi, first_chunk}: [lo, hi) of the flat buffer with lo a multiple of 4 elements and hi
   arbitrary (hi > lo); first_chunk = the sum of ceil((hi - lo) / VQA_STATS_CHUNK) over the rows before it, chunks = that sum over all
   rows.  The table is trusted as written, as the range tables of the optimizer are.  With d[i] = x[i] (y NULL) or x[i] - y[i] (one
   fp32 subtraction), row j of out -- P rows of four 32-bit words, 16-byte aligned -- is
     { sumsq (f32), absmax (f32), nonfinite (u32), zeros (u32) }
   nonfinite counts the d that are NaN or +-inf (inf - inf among them), zeros the d == 0 (-0.0 counts); sumsq and absmax run over the
   FINITE d only and are 0 when there is none.  Elements outside the rows are never read.
   Chunk c of a row is [lo + c * CHUNK, min(hi, lo + (c + 1) * CHUNK)); one 256-thread workgroup reduces one chunk in a fixed lane /
   wave order into scratch (device, 16-byte aligned, at least 4 * chunks words), a second launch folds each row's chunks in ascending
   order.  A row's four words are the same bits run to run and depend on (lo, hi) and the data alone: not on P, the grid, or the row's
   place in the table.  The counts and absmax are exact; sumsq is within N_add * 2^-24 relative of the exact sum (N_add: stats_ops.hip).
   Status 1000 without a launch: a NULL x, table, out or scratch; P outside 1 ... 4096; chunks < P or chunks >= 2^31. */
#define VQA_STATS_CHUNK 8192
int vqa_tensor_stats(const float* x, const float* y, const long long* table, int P, long long chunks, void* out, float* scratch,
                     hipStream_t stream);

/* ---- explaining an answer (csrc/explain_ops.hip; VQAModel.explain, Explanation.render) ----------------------------
 * All four accumulate in fp32 in a fixed order (no float atomics: the same bits on every run) and return status 1000 without a
 * launch for a NULL operand, a size < 1, a dtype other than 0 (fp32) / 1 (bf16) and the shapes named below.
 *
 * vqa_class_seed: the class whose score is explained, and the seed of its backward.  logits [B][N] in dtype (unit column stride,
 * row stride ld >= N); ids int64 [B] or NULL.
 *   chosen[b]     = ids[b], or without ids the arg-max of row b in vqa_softmax_topk's order: value descending, ties to the lower
 *                   index, a NaN ranks first -- chosen == the index vqa_softmax_topk(K = 1) returns
 *   dlogits[b][j] = 1 where j == chosen[b], else 0       ([B][N] contiguous, in the dtype of logits; an id outside [0, N) -- the
 *                   caller checks the range -- gives an all-zero row)
 * vqa_gradcam: Grad-CAM of NHWC features.  feat, dfeat [B][P][C] in dtype (16-byte aligned), cam fp32 [B][P].
 *   alpha[b][c] = (1/P) sum_p dfeat[b][p][c]
 *   cam[b][p]   = max(0, sum_c alpha[b][c] * feat[b][p][c])
 *   normalize != 0: cam[b][p] /= max_p cam[b][p] (a correctly rounded fp32 division; a row whose maximum is 0 stays all zero).
 *   One pass over each operand, one workgroup per image.  C must be a multiple of 8 and at most 1024.
 * vqa_attention_map: where the question looked.  caw fp32 [ncl][B][H][L][P] (the cross-attention probabilities of every layer in
 * one buffer), mask fp32 [B][L] (non-zero = real token) or NULL (every token is real), out fp32 [B][P].
 *   out[b][p] = (1 / (ncl * H * n_b)) sum_l sum_h sum_{t real} caw[l][b][h][t][p],  n_b = the number of real tokens of question b
 *   -- the mean over layers and heads of the reference's get_attention_visualization, averaged over the real tokens; each row sums
 *   to 1, and a question without a real token gives NaN (0 / 0), as its logits are.  normalize as in vqa_gradcam.  L * P <= 8192.
 * vqa_heatmap_render: a map as a picture.  map fp32 [B][Hm][Wm], base uint8 [B][H][W][3] or NULL, lut uint8 [256][3], out uint8
 * [B][H][W][3].  Per output pixel (y, x):
 *   t   = bilinear sample of map[b] at F.interpolate's align_corners=False source position: sy = max(0, (y + 0.5) * Hm / H - 0.5),
 *         rows y0 = floor(sy) and min(y0 + 1, Hm - 1) with weights 1 - (sy - y0) and sy - y0; columns likewise; fp32 throughout
 *   i   = clamp(floor(t * 255 + 0.5), 0, 255); a NaN t gives 0
 *   out = floor(alpha * lut[i][ch] + (1 - alpha) * base[b][y][x][ch] + 0.5) per channel, or lut[i][ch] without a base.
 *   alpha must lie in [0, 1]. */
int vqa_class_seed(int dtype, const void* logits, long long ld, const long long* ids, long long* chosen, void* dlogits, int B, int N,
                   hipStream_t stream);
int vqa_gradcam(int dtype, const void* feat, const void* dfeat, float* cam, int B, int P, int C, int normalize, hipStream_t stream);
int vqa_attention_map(const float* caw, const float* mask, float* out, int ncl, int B, int H, int L, int P, int normalize,
                      hipStream_t stream);
int vqa_heatmap_render(const float* map, const uint8_t* base, const uint8_t* lut, uint8_t* out, int B, int Hm, int Wm, int H, int W,
                       float alpha, hipStream_t stream);

/* ---- input pipeline on the GPU -----------------------------------------------------------------
 * vqa_image_normalize: torchvision ToTensor + Normalize of data/preprocess.py:34-35,117-121 -- uint8 HWC [B][H][W][3] ->
 * float32 NCHW, (u/255 - mean[c]) / std[c] in torch's operation order (bit-identical), optional per-sample horizontal flip
 * (flip[b] != 0; RandomHorizontalFlip, data/preprocess.py:73).  W % 4 == 0.
 * vqa_pack_tokens: Tokenizer.encode (utils/tokenizer.py:196-250) for a batch -- ragged vocabulary indices words[offsets[b] ..
 * offsets[b+1]) -> ids / mask int64 [B][L]: START + words + END, truncated to L with END forced onto the last slot, PAD after. */
/* vqa_image_resize: transforms.Resize((RH, RW)) of a PIL image (data/preprocess.py:70,90,118; api/inference.py:140-170), i.e.
 * PIL.Image.resize(BILINEAR) -- Pillow Resample.c restated bit-exactly (double-precision triangle weights scaled by the down-scale
 * factor, 22-bit fixed point, horizontal pass to a uint8 intermediate, then vertical) -- for a RAGGED batch: image i is uint8 HWC
 * [H[i]][W[i]][3] at in + in_off[i].  Optional RandomCrop window (crop_yx[2i], crop_yx[2i+1]) of size OH x OW inside the resized
 * RH x RW image (data/preprocess.py:70-71; NULL: no crop, then OH == RH and OW == RW) and per-sample horizontal flip (device
 * uint8[n] or NULL).  Outputs (either may be NULL): out_u8 [n][OH][OW][3] (what PIL returns) and out_nchw float32 [n][3][OH][OW] =
 * ToTensor + Normalize of it.  in_off / H / W / crop_yx are HOST arrays (they become kernel arguments, 32 images per launch);
 * `ws` is device scratch of vqa_image_resize_ws() bytes (coefficient tables + the horizontal intermediates). */
long long vqa_image_resize_ws(int n, const int* H, const int* W, int RH, int RW, int OW);
int vqa_image_resize(const uint8_t* in, const long long* in_off, const int* H, const int* W, const int* crop_yx, int n, int RH, int RW,
                     int OH, int OW, uint8_t* out_u8, float* out_nchw, const uint8_t* flip, float mean0, float mean1, float mean2,
                     float std0, float std1, float std2, void* ws, long long ws_bytes, hipStream_t stream);
/* vqa_image_color_jitter: transforms.ColorJitter (data/preprocess.py:77-82) of uint8 HWC images [B][H][W][3], fused with ToTensor +
 * Normalize.  On PIL images torchvision's adjustments are Pillow code -- ImageEnhance.Brightness / Contrast / Color =
 * Image.blend(black | rounded mean of the L band | L band, image, factor), hue = RGB -> HSV, H += delta (uint8 wrap), HSV -> RGB --
 * restated bit-exactly (libImaging Blend.c, Convert.c rgb2l / rgb2hsv_row / hsv2rgb: same float / double mix, no FMA contraction).
 * order: device uint8 [B][4], the permutation ColorJitter.forward draws (0 brightness, 1 contrast, 2 saturation, 3 hue; other values
 * are skipped).  factors: device float [B][4] = brightness, contrast, saturation factor and the hue DELTA int(hue_factor * 255) mod 256
 * as a float (the caller computes it in double, as torchvision does); NaN switches that adjustment off.  Outputs (either may be
 * NULL): out_u8 [B][H][W][3] (what PIL returns) and out_nchw float32 [B][3][H][W] = ToTensor + Normalize of it.
 * sums: device scratch of B 64-bit words (the L-band sums the contrast step needs; zeroed inside). */
int vqa_image_color_jitter(const uint8_t* in_hwc, const uint8_t* order, const float* factors, int B, int H, int W, uint8_t* out_u8,
                           float* out_nchw, float mean0, float mean1, float mean2, float std0, float std1, float std2,
                           unsigned long long* sums, hipStream_t stream);
int vqa_image_normalize(const uint8_t* in_hwc, float* out_nchw, const uint8_t* flip, int B, int H, int W, float mean0, float mean1,
                        float mean2, float std0, float std1, float std2, hipStream_t stream);
int vqa_pack_tokens(const int* words, const long long* offsets, long long* ids, long long* mask, int B, int L, int add_special,
                    int start_idx, int end_idx, int pad_idx, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
