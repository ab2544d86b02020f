/*
 * ocrs_hip.h -- C ABI of libocrs_hip.so, the MI355X (gfx950) implementation of the ocrs-models
 * detection / recognition train-step hot path.
 *
 * The reference (robertknight/ocrs-models) is pure PyTorch: its "FFI" for this path is the set of
 * torch.nn / torch.nn.functional calls made from ocrs_models/models.py, train_detection.py and
 * train_rec.py.  Each entry point below names the reference call site(s) it replaces.
 *
 * Conventions
 *   - plain pointers to DEVICE memory, sizes as int/long, a hipStream_t last; no torch types.
 *   - return 0 on success, 1 = bad argument, 2 = HIP launch/runtime error.  Nothing is allocated.
 *   - activations are NHWC ("[P][C]", P = N*H*W pixels), dtype: 0 = fp32, 1 = bf16 (raw uint16 bits).
 *     All arithmetic/accumulation is fp32; parameters, statistics and gradients of parameters are fp32.
 *   - "tr" arrays are per-channel load transforms [3][C] = scale | shift | lo, applied by every
 *     consumer as  x~ = max(x*scale + shift, lo)  (a producer's BatchNorm+ReLU, or identity 1|0|-inf).
 *   - functions that "accumulate" use atomics into a buffer the caller has zeroed.
 */
#ifndef OCRS_HIP_H
#define OCRS_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP_PLATFORM_AMD__
typedef struct ihipStream_t* hipStream_t;
#endif

/* ------------------------------------------------------------------ weight packing ---------- */
/* W[k][m] -> MFMA A-operand fragments.  mode 0: element at src[(k/K2)*s1 + (k%K2)*s2 + m*sm];
 * mode 1: ConvTranspose2d forward effective weight (src = W[Cup][Cout][3][3], K = 4*Cup, M = 4*Cout, K2 = Cup). */
int ocrs_pack_frags(const float* src, int mode, int K, int M, int K2, long s1, long s2, long sm, void* out, int dtype, hipStream_t st);
long ocrs_pack_frags_bytes(int K, int M, int dtype);
/* All weight packs of a step in one launch: table = device int64 [n][9] = { src, out, mode, K, M, K2, s1, s2, sm }. */
int ocrs_pack_frags_multi(const long long* table, int n, long max_frag_threads, int dtype, hipStream_t st);

/* ------------------------------------------------------------------ detection forward ------- */
/* DepthwiseConv block up to its pre-BatchNorm output: conv2d(groups=C, 3x3, pad 1) -> conv2d(1x1)
 * (ocrs_models/models.py:11-22) with the channel concat of models.py:89 folded in (xa|xb).
 * gstat [2][Cout] fp64 (sum z | sum z^2) is ACCUMULATED: the caller zeroes it (one memset for all layers of a step);
 * the same holds for gsum of ocrs_bn_bwd_reduce.
 * gamma / pooled (nullable; need ocrs_dwpw_fwd_pool_supported): also write nn.MaxPool2d(2) (models.py:54) of the block output in its
 * pre-BatchNorm form -- the z of each window's selected element (max z for gamma >= 0, min z for gamma < 0: relu(bn(.)) is monotone in z
 * with the sign of the BatchNorm weight) -- to pooled [N][H/2][W/2][Cout]; consumers read it through the block's load transform.
 */
int ocrs_dwpw_fwd(const void* xa, const void* xb, int Ca, int Cb, const float* tra, const float* trb, const float* wdw, const void* wpk,
                  void* z, double* gstat, const float* gamma, void* pooled, int Cout, int N, int H, int W, int dtype, hipStream_t st);
/* ocrs_dwpw_fwd + ocrs_bn_finalize in one launch (models.py:11-23 for the deep levels, 32..256 channels in bf16): the last workgroup done finalises
   the BatchNorm statistics.  counter: a zeroed device word (left zeroed); count .. lo as ocrs_bn_finalize.  No fused pooling. */
long ocrs_dwpw_fwd_fin_supported(int Cin, int Cout, int dtype);
int ocrs_dwpw_fwd_fin(const void* xa, const void* xb, int Ca, int Cb, const float* tra, const float* trb, const float* wdw, const void* wpk, void* z,
                      double* gstat, unsigned* counter, long count, const float* bn_w, const float* bn_b, float eps, float momentum, float* tr, float* saved,
                      float* run_mean, float* run_var, long long* nbt, float lo, int Cout, int N, int H, int W, int dtype, hipStream_t st);
long ocrs_dwpw_fwd_pool_supported(int Cin, int Cout); /* 1 / 0 */
/* The same block forward in fp32 -- the reference's own arithmetic (train_detection.py:92-97 runs models.py:11-23 without autocast) -- as
 * register-resident row-streaming waves (csrc/det_rs32.hip, round 6): Cin = Ca + Cb in {8, 16, 32} (concat only as 8 | 8 or 16 | 16), Cout in
 * {8, 16, 32}; depthwise on the VALU with DPP neighbours, pointwise on the exact-fp32 matrix cores (v_mfma_f32_16x16x4_f32), no LDS tile.
 * wdw [Cin][9], wpw [Cout][Cin]: the fp32 masters in the reference layout.  gstat / gamma / pooled: as ocrs_dwpw_fwd.  counter (nullable: then
 * count .. lo are ignored and the caller runs ocrs_bn_finalize): a zeroed device word (left zeroed) -- the launch's last workgroup finalises the
 * BatchNorm statistics exactly as ocrs_bn_finalize does. */
long ocrs_rs32_fwd_supported(int Ca, int Cb, int Cout, int dtype); /* 1 / 0 */
int ocrs_rs32_fwd(const float* xa, const float* xb, int Ca, int Cb, const float* tra, const float* trb, const float* wdw, const float* wpw, float* z,
                  double* gstat, const float* gamma, float* pooled, unsigned* counter, long count, const float* bn_w, const float* bn_b, float eps,
                  float momentum, float* tr, float* saved, float* run_mean, float* run_var, long long* nbt, float lo, int Cout, int N, int H, int W,
                  hipStream_t st);
/* Backward of the same block in fp32 as ONE row-streaming pass (csrc/det_rs32.hip; the autograd of models.py:11-23 as train_detection.py:96 runs it):
 * replaces ocrs_bn_bwd_finalize + ocrs_pw_bwd + ocrs_dw_bwd -- per pixel g (+ g2), z and x are read once and dL/dx~ is written once, the depthwise-input
 * gradient `du` never goes to memory.  Cin = Ca + Cb in {8, 16} (concat 8 | 8), Cout in {8, 16}; of level 1 also 16 | 16 -> 16 (two single-source passes)
 * and 16 -> 32.
 * pooled = 1 (single source only): g1 / g2 are at half resolution and routed through MaxPool2d(2) (models.py:54) to each window's first maximum.
 * gsum [2][Cout] fp64: the block's COMPLETE BatchNorm-backward sums (the dz coefficients are derived in the prologue; dgamma / dbeta are written);
 * bn: the block's load transform [3][Cout]; dwpw / dwdw ACCUMULATED through ws (ocrs_rs32_bwd_ws_floats() floats; alive until ocrs_bwd_defer_flush
 * when a deferral window is open); saved_a / gsum_a, saved_b / gsum_b (nullable): as ocrs_dw_bwd. */
long ocrs_rs32_bwd_supported(int Ca, int Cb, int Cout, int pooled, int dtype); /* 1 / 0 */
long ocrs_rs32_bwd_ws_floats(int Ca, int Cb, int Cout, int N, int H, int W);
int ocrs_rs32_bwd(const float* xa, const float* xb, int Ca, int Cb, const float* tra, const float* trb, const float* wdw, const float* wpw, const float* g1,
                  const float* g2, const float* z, const float* bn, const double* gsum, const float* gamma, const float* saved, float* dgamma, float* dbeta,
                  float* gxa, float* gxb, float* dwpw, float* dwdw, float* ws, const float* saved_a, double* gsum_a, const float* saved_b, double* gsum_b,
                  int pooled, int Cout, int N, int H, int W, hipStream_t st);
/* ocrs_rs32_bwd for the block in front of out_conv (models.py:125-129; 8 -> 8, single source): its output gradient is formed on the fly,
   g[p][c] = gl[p] * whead[c], from out_conv's dL/dlogit gl [P] fp32 (what ocrs_head_bwd_gl / ocrs_head_bwd_loss write: 4 instead of 32 bytes per pixel) -- the same
   fp32 product ocrs_head_bwd stores, so every output is bit-identical to ocrs_head_bwd + ocrs_rs32_bwd. */
long ocrs_rs32_bwd_head_supported(int Ca, int Cb, int Cout, int dtype); /* 1 / 0 */
int ocrs_rs32_bwd_head(const float* xa, int Ca, const float* tra, const float* wdw, const float* wpw, const float* gl, const float* whead, const float* z,
                       const float* bn, const double* gsum, const float* gamma, const float* saved, float* dgamma, float* dbeta, float* gxa, float* dwpw,
                       float* dwdw, float* ws, const float* saved_a, double* gsum_a, int Cout, int N, int H, int W, hipStream_t st);
/* The same block forward on the matrix cores (csrc/det_mm.hip; bf16, Cin and Cout in {8, 16, 32} and the 32 | 32 concat): depthwise and
 * pointwise conv composed into one 3x3 implicit GEMM (effective weight Wpw[o][c] * Wdw[c][tap] built from the fp32 masters wdw [Cin][9],
 * wpw [Cout][Cin]).  The batch statistics go to ws as ocrs_mm_fwd_nparts() per-block partials [Cout][sum z | sum z^2] (fp32) that
 * ocrs_bn_finalize_parts reduces in a fixed order (bit-reproducible; no atomics).  gamma / pooled: as ocrs_dwpw_fwd. */
long ocrs_mm_fwd_supported(int Ca, int Cb, int Cout, int dtype); /* 1 / 0 */
long ocrs_mm_fwd_nparts(int Ca, int Cb, int Cout, int N, int H, int W);
int ocrs_mm_fwd(const void* xa, const void* xb, int Ca, int Cb, const float* tra, const float* trb, const float* wdw, const float* wpw, void* z,
                float* ws, const float* gamma, void* pooled, int Cout, int N, int H, int W, int dtype, hipStream_t st);
/* ocrs_mm_fwd with ocrs_bn_finalize_parts folded into the same launch (models.py:11-24: conv + BatchNorm2d training statistics; the last workgroup to
   finish reduces the per-block partials in the association order of ocrs_bn_finalize_parts: bit-identical tr / saved / running statistics).
   counter: one zeroed 32-bit word (left zero); bn_w / bn_b: the block's BatchNorm weight / bias; count, eps, momentum, tr, saved, run_mean,
   run_var, nbt, lo: as ocrs_bn_finalize_parts. */
int ocrs_mm_fwd_fin(const void* xa, const void* xb, int Ca, int Cb, const float* tra, const float* trb, const float* wdw, const float* wpw, void* z, float* ws,
                    const float* gamma, void* pooled, unsigned* counter, long count, const float* bn_w, const float* bn_b, float eps, float momentum, float* tr,
                    float* saved, float* run_mean, float* run_var, long long* nbt, float lo, int Cout, int N, int H, int W, int dtype, hipStream_t st);
/* ocrs_mm_fwd_fin for the block behind the first block (models.py:115, in_conv's second DepthwiseConv): the input is given as the first block's u plane
   (ocrs_dwpw_c1_fwd_u) and pointwise weight wexp [8]; tra = the first block's load transform [3][8].  No pooling. */
int ocrs_mm_fwd_fin_xu(const void* xu, const float* wexp, const float* tra, const float* wdw, const float* wpw, void* z, float* ws, unsigned* counter, long count,
                       const float* bn_w, const float* bn_b, float eps, float momentum, float* tr, float* saved, float* run_mean, float* run_var, long long* nbt,
                       float lo, int Cout, int N, int H, int W, int dtype, hipStream_t st);
int ocrs_bn_finalize_parts(const float* parts, int nparts, long count, int C, const float* gamma, const float* beta, float eps, float momentum,
                           float* tr, float* saved, float* run_mean, float* run_var, long long* nbt, float lo, hipStream_t st);
/* Same for the first block (1 -> 8 channels, models.py:115) reading the fp32 image (N,1,H,W). */
int ocrs_dwpw_c1_fwd(const float* img, const float* wdw, const float* wpw, void* z, double* gstat, int N, int H, int W, int dtype,
                     hipStream_t st);
/* The same first block (models.py:115: in_conv's DepthwiseConv(1, 8)), additionally writing uplane [N][H][W] bf16 = its rounded depthwise output u: the block
   output is rank one over the channels, z[p][c] = round(wpw[c] * u[p]), so consumers that take the u plane (ocrs_mm_bwd_fin_xu) read 2 instead of 16
   bytes per pixel.  ocrs_dwpw_c1_u_supported: 1 / 0. */
long ocrs_dwpw_c1_u_supported(int N, int H, int W, int dtype);
int ocrs_dwpw_c1_fwd_u(const float* img, const float* wdw, const float* wpw, void* z, void* uplane, double* gstat, int N, int H, int W, int dtype,
                       hipStream_t st);
/* nn.BatchNorm2d training statistics (models.py:23): sums -> tr [3][C], saved mean|rstd [2][C], running stats, num_batches_tracked. */
int ocrs_bn_finalize(const double* gstat, long count, int C, const float* gamma, const float* beta, float eps, float momentum, float* tr,
                     float* saved, float* run_mean, float* run_var, long long* nbt, float lo, hipStream_t st);
/* nn.MaxPool2d(2) (models.py:54) over relu(bn(z)).  raw = 0: out = the window maximum; raw = 1: out = the pre-BatchNorm z of the selected
 * element (first maximum), to be consumed through the producer's load transform `tr` like any block output. */
int ocrs_maxpool_fwd(const void* z, const float* tr, void* out, int C, int N, int H, int W, int raw, int dtype, hipStream_t st);
/* nn.ConvTranspose2d(k=3, s=2) + crop (models.py:76-78, 82-87). */
int ocrs_convt_fwd(const void* x, const float* tr, const void* wpk, const float* bias, void* out, int Cup, int Cout, int N, int h, int w,
                   int H, int W, int dtype, hipStream_t st);
/* The same ConvTranspose2d forward in fp32 as row-streaming waves over the input grid (csrc/det_rs32.hip, round 6): (Cup, Cout) in {(16, 8), (32, 16),
   (32, 32)}; wt = the fp32 MASTER weight [Cup][Cout][3][3] (no packed fragments: the effective per-parity fragments are built in LDS per workgroup). */
long ocrs_rs32_convt_fwd_supported(int Cup, int Cout, int dtype); /* 1 / 0 */
int ocrs_rs32_convt_fwd(const float* x, const float* tr, const float* wt, const float* bias, float* out, int Cup, int Cout, int N, int h, int w, int H, int W,
                        hipStream_t st);
/* ... and its input gradient (the dx half of ocrs_convt_bwd_parts; autograd of models.py:76-78) in fp32 as row-streaming waves over the input grid, (Cup, Cout)
   in {(16, 8), (32, 16)}, from the MASTER weight; x / tr / saved / gsum (nullable together): also the BatchNorm-backward sums of the block that produced x when
   this ConvTranspose is its only consumer (as ocrs_convt_bwd's saved / gsum: [2][Cup] fp64, ACCUMULATED). */
long ocrs_rs32_convt_dgrad_supported(int Cup, int Cout, int dtype); /* 1 / 0 */
int ocrs_rs32_convt_dgrad(const float* g, const float* wt, float* dx, const float* x, const float* tr, const float* saved, double* gsum, int Cup, int Cout, int N,
                          int h, int w, int H, int W, hipStream_t st);
/* out_conv: nn.Conv2d(8, 1, 1) + nn.Sigmoid (models.py:125-129). */
int ocrs_head_fwd(const void* z, const float* tr, const float* w, const float* b, float* pred, long P, int dtype, hipStream_t st);

/* ------------------------------------------------------------------ detection backward ------ */
/* autograd of BatchNorm2d+ReLU (+MaxPool2d when pooled=1): reductions, then per-channel dz coefficients + dgamma/dbeta. */
int ocrs_bn_bwd_reduce(const void* g1, const void* g2, int pooled, const void* z, const float* bn, const float* saved, double* gsum, int C,
                       int N, int H, int W, int dtype, hipStream_t st);
int ocrs_bn_bwd_finalize(const double* gsum, long count, int C, const float* gamma, const float* saved, float* coef, float* dgamma,
                         float* dbeta, hipStream_t st);
/* autograd of the 1x1 conv (dgrad written to du, wgrad accumulated into dwpw [Cout][Cin]). */
/*   ws: ocrs_pw_bwd_ws_floats() floats of workspace (per-block partials, deterministic two-stage reduction) or NULL (float atomics).  Inside a
 *   deferral window (ocrs_bwd_defer_begin) kernels 1-3 of ocrs_pw_bwd_kernel queue that reduction until ocrs_bwd_defer_flush -- ws must stay alive
 *   until then -- except the first of kernel 3's two launches, which share ws; kernel 4 always reduces at once. */
long ocrs_pw_bwd_ws_floats(int Cin, int Cout, int N, int H, int W);
int ocrs_pw_bwd(const void* xa, const void* xb, int Ca, int Cb, const float* tra, const float* trb, const float* wdw, const void* g1,
                const void* g2, int pooled, const void* z, const float* bn, const float* coef, const void* wpk_d, void* du, float* dwpw,
                float* ws, int Cout, int N, int H, int W, int dtype, hipStream_t st);
/* ocrs_bn_bwd_finalize + ocrs_pw_bwd in one call (the deep-level bf16 kernel folds the finalisation into its prologue): gsum [2][Cout] fp64 complete
   sums of this block, gamma, saved [mean | rstd]; dgamma / dbeta written; coef [3][Cout] is scratch. */
int ocrs_pw_bwd_fin(const void* xa, const void* xb, int Ca, int Cb, const float* tra, const float* trb, const float* wdw, const void* g1, const void* g2,
                    int pooled, const void* z, const float* bn, float* coef, const double* gsum, const float* gamma, const float* saved, float* dgamma,
                    float* dbeta, const void* wpk_d, void* du, float* dwpw, float* ws, int Cout, int N, int H, int W, int dtype, hipStream_t st);
/* the kernel ocrs_pw_bwd_fin runs for a block shape when given a workspace: 1 = k_pwb (det_pwb.hip), 2 = k_pw_bwd2 (det_pw2.hip), 3 = k_pw_bwd2
   once per source of a 32 | 32 concat, 4 = the generic k_pw_bwd, 0 = none (the call answers OCRS_ERR_ARG) */
long ocrs_pw_bwd_kernel(int Ca, int Cb, int Cout, int dtype);
/* autograd of the depthwise 3x3 conv (dL/dx~ split at channel Ca into gxa|gxb; dwdw [C][1][3][3] accumulated). */
/*   ws: ocrs_dw_bwd_ws_floats() floats of workspace (per-block partials, two-stage reduction) or NULL (float atomics). */
long ocrs_dw_bwd_ws_floats(int C, int N, int H, int W);
/*   gsum_a / gsum_b (nullable, need ws): ALSO accumulate the BatchNorm-backward sums [sum ghat | sum ghat*zhat] ([2][Ca] / [2][Cb] fp64,
 *   zeroed by the caller before the first consumer) of the blocks that produced source a / b -- this replaces their ocrs_bn_bwd_reduce
 *   when every consumer of that block output is a depthwise conv; saved_a / saved_b = those blocks' saved [mean | rstd]. */
int ocrs_dw_bwd(const void* xa, const void* xb, int Ca, int Cb, const float* tra, const float* trb, const float* wdw, const void* du,
                void* gxa, void* gxb, float* dwdw, float* ws, const float* saved_a, double* gsum_a, const float* saved_b, double* gsum_b,
                int N, int H, int W, int dtype, hipStream_t st);
/* The same block backward on the matrix cores (csrc/det_mm.hip; bf16, Cin and Cout in {8, 16, 32}, a 32 | 32 concat as two launches):
 * depthwise and pointwise conv composed into one 3x3 implicit GEMM with the effective weight Wpw[o][c] * Wdw[c][tap]; replaces
 * ocrs_pw_bwd + ocrs_dw_bwd (autograd of models.py:12-22 through BatchNorm2d + ReLU [+ MaxPool2d(2) when pooled], models.py:23-24, 54) -- the
 * pointwise input gradient du is never formed.  wdw [Cin][9] / wpw [Cout][Cin]: fp32 master weights; g1 (+ g2) at half resolution when
 * pooled = 1; dwpw / dwdw are ACCUMULATED by a single writer per element (deterministic, no atomics); ws = ocrs_mm_bwd_ws_floats() floats;
 * saved_a / gsum_a, saved_b / gsum_b: as ocrs_dw_bwd (nullable). */
long ocrs_mm_bwd_supported(int Ca, int Cb, int Cout, int dtype); /* 1 / 0 */
long ocrs_mm_bwd_ws_floats(int Ca, int Cb, int Cout, int N, int H, int W);
/* nb, the number of per-block partials ONE launch of the block backward leaves in ws (every entry point of this family; 0: unsupported shape).
 * Partial b is ws[b * ne .. (b + 1) * ne), ne = Cout * Cin + 11 * Cin floats:  [Cout][Cin] dWpw | [Cin][9] dWdw | [Cin][S1 | S2] interleaved, the
 * launch's share of S1 = sum ghat', S2 = sum ghat' x~ over its pixels (ghat' = dL/dx~ where x~ > 0; defined only when gsum_a / gsum_b ask for sums).  They stay
 * in ws after the launch and after its reduction.  A 32 | 32 concat input runs as two launches of Cin = 32 (source a, then b): nb is the per-launch
 * value and the second launch's partials start at float nb * (Cout * 32 + 11 * 32 + 1024) of ws.  two_grads: g2 != NULL. */
long ocrs_mm_bwd_nparts(int Ca, int Cb, int Cout, int pooled, int two_grads, int N, int H, int W);
int ocrs_mm_bwd(const void* xa, const void* xb, int Ca, int Cb, const float* tra, const float* trb, const float* wdw, const float* wpw,
                const void* g1, const void* g2, int pooled, const void* z, const float* bn, const float* coef, void* gxa, void* gxb, float* dwpw,
                float* dwdw, float* ws, const float* saved_a, double* gsum_a, const float* saved_b, double* gsum_b, int Cout, int N, int H,
                int W, int dtype, hipStream_t st);
/* ocrs_mm_bwd with ocrs_bn_bwd_finalize folded into the kernel prologue: instead of `coef`, this block's complete BatchNorm-backward sums gsum [2][Cout]
   (fp64), gamma and saved [mean | rstd]; dgamma / dbeta [Cout] are written (models.py:23 backward). */
int ocrs_mm_bwd_fin(const void* xa, const void* xb, int Ca, int Cb, const float* tra, const float* trb, const float* wdw, const float* wpw, const void* g1,
                    const void* g2, int pooled, const void* z, const float* bn, const double* gsum, const float* gamma, const float* saved, float* dgamma,
                    float* dbeta, void* gxa, void* gxb, float* dwpw, float* dwdw, float* ws, const float* saved_a, double* gsum_a, const float* saved_b,
                    double* gsum_b, int Cout, int N, int H, int W, int dtype, hipStream_t st);
/* ocrs_mm_bwd_fin for the block in front of out_conv (models.py:143 reads up.0.contract's output): the gradient w.r.t. the block output is
   not read from memory but formed as round(gl[p] * whead[c]) from ocrs_head_bwd_gl's 4-byte-per-pixel gl.  ocrs_mm_bwd_head_supported: 1 if this
   launch is covered (the row-streaming backward: bf16, 8 -> 8 channels, one source). */
long ocrs_mm_bwd_head_supported(int Ca, int Cb, int Cout, int N, int H, int W, int dtype);
int ocrs_mm_bwd_fin_head(const void* xa, int Ca, const float* tra, const float* wdw, const float* wpw, const float* gl, const float* whead, const void* z,
                         const float* bn, const double* gsum, const float* gamma, const float* saved, float* dgamma, float* dbeta, void* gxa, float* dwpw,
                         float* dwdw, float* ws, const float* saved_a, double* gsum_a, int Cout, int N, int H, int W, int dtype, hipStream_t st);
/* ocrs_mm_bwd_fin for the block behind the first block (models.py:115: in_conv's second DepthwiseConv): its input is given as the first block's u plane
   (ocrs_dwpw_c1_fwd_u) and pointwise weight wexp [8] -- x[p][c] = round(wexp[c] * u[p]), the stored values, rebuilt from 2 instead of 16 bytes per pixel.
   Needs ocrs_mm_bwd_head_supported(8, 0, Cout, ...). */
int ocrs_mm_bwd_fin_xu(const void* xu, const float* wexp, const float* tra, const float* wdw, const float* wpw, const void* g1, const void* g2, const void* z,
                       const float* bn, const double* gsum, const float* gamma, const float* saved, float* dgamma, float* dbeta, void* gxa, float* dwpw,
                       float* dwdw, float* ws, const float* saved_a, double* gsum_a, int Cout, int N, int H, int W, int dtype, hipStream_t st);
/* acc64 [17] fp64 = dWpw [8] | dWdw [9], ACCUMULATED (caller-zeroed; the caller adds it to the fp32 gradients): fp64 sums of the per-block
 * fp32 partials are exact, hence independent of the order the blocks finish in (float atomics into the fp32 gradients were not). */
int ocrs_dwpw_c1_bwd(const float* img, const float* wdw, const float* wpw, const void* g1, const void* g2, int pooled, const void* z,
                     const float* bn, const float* coef, double* acc64, int N, int H, int W, int dtype, hipStream_t st);
/* autograd of ConvTranspose2d + crop. */
long ocrs_convt_bwd_ws_floats(int Cup, int Cout, int N, int h, int w, int dtype);
/* saved / gsum (nullable; need ocrs_convt_bwd_stats_supported): x is the raw output of a block consumed ONLY by this ConvTranspose -> its
 * BatchNorm-backward sums [2][Cup] (fp64, ACCUMULATED; saved = the block's [mean | rstd]) come from this pass instead of ocrs_bn_bwd_reduce. */
/* dbias64 [Cout] fp64 (caller-zeroed): where the generic (deep-level) path accumulates the bias gradient; the caller adds it to dbias.  The tiled
 * bf16 path of levels 0-2 adds the bias gradient to dbias itself, and so does fp32 with a workspace, Cup in {16, 32} and Cout in {8, 16, 32} (the
 * row-streaming weight-gradient kernel, csrc/det_rs32.hip): dbias64 then stays as the caller zeroed it.
 * ws: ocrs_convt_bwd_ws_floats() floats.  Inside a deferral window (ocrs_bwd_defer_begin) the row-streaming kernel queues its reduction of ws into
 * dW / dbias until ocrs_bwd_defer_flush: ws must stay alive until the flush, and dW / dbias are complete only after it.
 * All of this holds for the weight + bias half (parts & 2) of ocrs_convt_bwd_parts as well. */
int ocrs_convt_bwd(const void* x, const float* tr, const void* g, const void* wpk_d, void* dx, float* dW, float* dbias, double* dbias64, float* ws,
                   const float* saved, double* gsum, int Cup, int Cout, int N, int h, int w, int H, int W, int dtype, hipStream_t st);
long ocrs_convt_bwd_stats_supported(int Cup, int Cout, int dtype); /* 1 / 0 */
/* The same pass in two calls -- parts bit 0: input gradient dx; bit 1: weight + bias gradients (off the backward's critical path: may run on another
 * stream) -- where ocrs_convt_bwd_splittable() (the generic deep-level path; the tiled path of levels 0-2 needs parts == 3). */
long ocrs_convt_bwd_splittable(int Cup, int Cout, int dtype);
int ocrs_convt_bwd_parts(const void* x, const float* tr, const void* g, const void* wpk_d, void* dx, float* dW, float* dbias, double* dbias64, float* ws,
                         const float* saved, double* gsum, int Cup, int Cout, int N, int h, int w, int H, int W, int parts, int dtype, hipStream_t st);
/* Fused first-block backward (round 5; models.py:115 in_conv = DoubleConv(1, 8): the backward of its first DepthwiseConv block).  The block's weight gradient is
   linear in dL/dx~ of its only consumer, so ocrs_mm_bwd_fin_xu_c1 -- ocrs_mm_bwd_fin_xu for in_conv.seq.1 -- accumulates, instead of storing dL/dx~ (16 B / pixel),
   the sums c1acc [8][32] fp64 (caller-zeroed: R[c] = sum ghat1[c] u, T[tap] = sum (sum_c wexp[c] A[c] ghat1[c]) img(tap), 8 replicas) from the network input
   img [N H W] fp32; ocrs_dwpw_c1_fwd_us is ocrs_dwpw_c1_fwd_u that also accumulates the forward-only sums fsum [20] fp64 (caller-zeroed: sum u | sum u^2 |
   sum u img(tap) [9] | sum img(tap) [9]); ocrs_c1_bwd_fin combines both with the block's BatchNorm-backward coefficients coef [3][8] (ocrs_bn_bwd_finalize)
   into acc64 [17] += dWpw [8] | dWdw [9] -- the output of ocrs_dwpw_c1_bwd, which is then not needed. */
int ocrs_dwpw_c1_fwd_us(const float* img, const float* wdw, const float* wpw, void* z, void* uplane, double* gstat, double* fsum, int N, int H, int W, int dtype,
                        hipStream_t st);
int ocrs_mm_bwd_fin_xu_c1(const void* xu, const float* wexp, const float* tra, const float* wdw, const float* wpw, const void* g1, const void* g2, const void* z,
                          const float* bn, const double* gsum, const float* gamma, const float* saved, float* dgamma, float* dbeta, float* dwpw, float* dwdw,
                          float* ws, const float* saved_a, double* gsum_a, const float* img, double* c1acc, int Cout, int N, int H, int W, int dtype,
                          hipStream_t st);
int ocrs_c1_bwd_fin(const double* c1acc, const double* fsum, const float* coef, const float* wexp, double* acc64, hipStream_t st);
/* Deferred second stage of the block backward (models.py:7-28 backward; no reference counterpart -- it is launch scheduling): between _begin and _flush
   the block-backward entry points (ocrs_mm_bwd*, ocrs_pw_bwd*, ocrs_dw_bwd) (1) finalise the BatchNorm-backward sums they produce for their input's
   producers (gsum_a / gsum_b) in the last workgroup of the block kernel, using state carved from `scratch` (ndoubles ZEROED fp64 values, left zeroed),
   and (2) queue the single-writer reductions of their weight-gradient partials instead of launching them; _flush launches all queued reductions as
   ONE kernel on `st` and ends the mode.  `scratch` and every workspace `ws` passed meanwhile must stay valid until _flush has been queued; dwpw /
   dwdw are complete only after it.  Results are bit-identical to the undeferred launches except for the gsum sums (exact fp64 sums of the fp32
   per-block partials instead of fp32 chain sums).  Per-process state: one backward at a time. */
int ocrs_bwd_defer_begin(double* scratch, long ndoubles);
int ocrs_bwd_defer_flush(hipStream_t st);
/* autograd of out_conv + sigmoid. */
/* acc64 [9] fp64 = dw [8] | db, ACCUMULATED (caller-zeroed, caller adds it to the fp32 gradients; see ocrs_dwpw_c1_bwd). */
int ocrs_head_bwd(const void* z, const float* tr, const float* w, const float* pred, const float* gpred, void* gy, double* acc64,
                  const float* saved, double* gsum, long P, int dtype, hipStream_t st);
/* The same (models.py:127-130, 143: out_conv + Sigmoid backward) with a compact output: gl [P] fp32 = dL/dlogit instead of the 8-channel gradient gy
   (gy[p][c] = gl[p] * w[c] is formed by the consumer, ocrs_mm_bwd_fin_head). */
int ocrs_head_bwd_gl(const void* z, const float* tr, const float* w, const float* pred, const float* gpred, float* gl, double* acc64,
                     const float* saved, double* gsum, long P, int dtype, hipStream_t st);
/* ocrs_balanced_bce_bwd + ocrs_head_bwd_gl in one pass (the autograd of train_detection.py:225-263's loss followed by models.py:143's out_conv + Sigmoid
   backward): dL/dpred is formed on the fly from what ocrs_balanced_bce_fwd saved (pred, target, lpx, cls, state) and gout [1], the upstream gradient
   of the scalar loss; it is never written to memory.  P % 4 == 0; saved / gsum as ocrs_head_bwd (required). */
int ocrs_head_bwd_loss(const void* z, const float* tr, const float* w, const float* pred, const float* target, const float* lpx, const unsigned char* cls,
                       const void* state, const float* gout, float* gl, double* acc64, const float* saved, double* gsum, long P, int dtype,
                       hipStream_t st);

/* ------------------------------------------------------------------ detection loss ---------- */
/* balanced_cross_entropy_loss (ocrs_models/train_detection.py:225-263), forward and backward. */
long ocrs_loss_state_bytes(void);
long ocrs_loss_hist_bytes(void);
int ocrs_balanced_bce_fwd(const float* pred, const float* target, float* lpx, unsigned char* cls, void* state, void* hist, float* loss_out,
                          long P, hipStream_t st);
int ocrs_balanced_bce_bwd(const float* pred, const float* target, const float* lpx, const unsigned char* cls, const void* state,
                          const float* gout, float* gpred, long P, hipStream_t st);
/* dst[table[r][0] + i] += src[table[r][1] + i], i < table[r][2], r < nrows (table: int32 [nrows][3], device): the ~10 fp64 accumulator folds of a
   detection backward (out_conv / first-block weights, ConvTranspose biases: ocrs_models/models.py:93-143 autograd) in one launch. */
int ocrs_fold64_multi(const int* table, int nrows, float* dst, const double* src, hipStream_t st);

/* ------------------------------------------------------------------ recognition (CRNN) ------ */
/* nn.Conv2d forward / dgrad, GRU input projections, nn.Linear as one implicit-GEMM kernel (ocrs_models/models.py:189-240, 245, 248).
 * gstat (nullable) [2][M] fp64 (sum z | sum z^2 of the stored outputs) is ACCUMULATED: the caller zeroes it (one fill for all layers of a
 * step); the same holds for gsum of ocrs_rec_bn_reduce / ocrs_avgpool_bn_reduce. */
int ocrs_conv_igemm(const void* x, int ldx, const void* wpk, void* out, int ldo, const float* bias, int relu, double* gstat, int Cin, int M, int N,
                    int Hi, int Wi, int Ho, int Wo, int KH, int KW, int padh, int padw, int dtype, hipStream_t st);
/* the kernel ocrs_conv_igemm runs for these arguments: 1 = k_conv3x3_tile, 2 = k_conv3x3_rows, 3 = k_conv3x3_c128, 0 = the generic k_conv_igemm */
long ocrs_conv_igemm_kernel(int ldx, int ldo, int Cin, int M, int Hi, int Wi, int Ho, int Wo, int KH, int KW, int padh, int padw, int dtype);
/* weight gradients of Conv2d / Linear / GRU (autograd of the calls above). */
/* Split-bf16 (bf16x3) weight-gradient GEMM for fp32 operands: dW [CA][CB] += A^T B over P rows (throughput mode of the GRU / Linear
 * weight gradients, train_rec.py:140 backward of models.py:264-268); <= ~1.1e-5 relative error per product, fp32 accumulation.
 * CB % 4 == 0; CA may be ragged (the class count) when ldA >= round_up(CA, 4). */
long ocrs_wgrad_gemm_x3_ws_floats(int CA, int CB, long P);
int ocrs_wgrad_gemm_x3(const float* A, int ldA, int CA, const float* B, int ldB, int CB, float* dW, float* ws, long P, hipStream_t st);
/* Split-bf16 GEMM for fp32 operands (GRU input projections and their input gradients in throughput mode, models.py:264-266):
 * out [P][ldo] = X [P][ldx] (K columns) * W (+ bias), W[m][k] = Wm[m * ldw + k] (km = 0) or Wm[k * ldw + m] (km = 1).
 * Kw (0: K): the k extent Wm really has; X columns [Kw, K) meet zero weights.  km = 0 also takes M % 4 != 0 (nn.Linear(512, n_classes) and
 * its input gradient, models.py:245-248): output columns [M, round_up(M, 4)) are written as 0. */
int ocrs_gemm_x3(const float* X, int ldx, int K, const float* Wm, int ldw, int km, const float* bias, float* out, int ldo, int M, long P, int Kw,
                 hipStream_t st);
/* The pipelined form of the same GEMM (csrc/rec_gemm.hip, round 4: one workgroup per CU = 8 MFMA waves + 4 producer waves that move both
 * operands by LDS-DMA through a three-stage ring, persistent over XCD-ordered tiles).  Weights pre-split and pre-packed once per step:
 * wpk = ocrs_pack_frags(mode 2, dtype 1) of W as A[m][k], 2 * ocrs_pack_frags_bytes(K, M, 1) bytes.  K % 32 == 0, M % 128 == 0, M <= 2048,
 * P * ldx * 4 < 2^31 -- ocrs_gemm_x3p_supported() returns 1 for shapes it takes.  Bit-identical to ocrs_gemm_x3. */
long ocrs_gemm_x3p_supported(int ldx, int K, int ldo, int M, long P);
int ocrs_gemm_x3p(const float* X, int ldx, int K, const void* wpk, const float* bias, float* out, int ldo, int M, long P, hipStream_t st);
/* ... with the workgroup tile height chosen by the caller: ntw = 4 (256 rows), 2 (128 rows) or 0 (automatic, what ocrs_gemm_x3p does). */
int ocrs_gemm_x3p_tiles(const float* X, int ldx, int K, const void* wpk, const float* bias, float* out, int ldo, int M, long P, int ntw, hipStream_t st);
long ocrs_wgrad_gather_ws_floats(int CA, int CB, int ntaps, long P, int dtype);
int ocrs_wgrad_gather(const void* A, int ldA, int CA, const float* trA, const void* B, int ldB, int CB, float* dW, float* ws, int N, int hA,
                      int wA, int HB, int WB, int stride, int padh, int padw, int KH, int KW, int dtype, hipStream_t st);
/* weight gradient of the 3x3 / pad 1 Conv2d layers (models.py:189-231), all nine taps per staged tile. */
long ocrs_conv3x3_wgrad_ws_floats(int Cout, int Cin, int N, int H, int W);
int ocrs_conv3x3_wgrad(const void* dz, int Cout, const void* x, int Cin, float* dW, float* ws, int N, int H, int W, int dtype, hipStream_t st);
/* Conv2d(1,32,3,p1) + ReLU + MaxPool2d(2) (models.py:180-187) fused, forward and backward. */
int ocrs_conv0_fwd(const float* img, const float* w, const float* bias, void* out, int N, int H, int W, int dtype, hipStream_t st);
int ocrs_conv0_bwd(const float* img, const float* w, const float* bias, const void* g, float* dW, float* db, int N, int H, int W, int dtype,
                   hipStream_t st);
/* BatchNorm2d + ReLU + MaxPool2d((2,2)|(2,1)) (models.py:197-199, 214-216, 231-233) forward and the pieces of its backward.
 * Windows (PH, PW) = (2,2), (2,1) or (1,1) (no pooling), floor mode: a last row / column that H % PH or W % PW leaves over is in no window
 * (ocrs_dz_apply gives its pixels coefB*z + coefC).  C / 8 must be a power of two <= 256.  Anything else returns 1 and launches nothing. */
int ocrs_act_pool_fwd(const void* z, const float* tr, void* out, int C, int N, int H, int W, int PH, int PW, int dtype, hipStream_t st);
int ocrs_rec_bn_reduce(const void* g, const void* z, const float* bn, const float* saved, double* gsum, int C, int N, int H, int W, int PH, int PW,
                       int dtype, hipStream_t st);
int ocrs_dz_apply(const void* g, const void* z, const float* bn, const float* coef, void* dz, int C, int N, int H, int W, int PH, int PW, int dtype,
                  float* dsum /* nullable [C]: += column sums of dz (the bias gradient of a biased conv, models.py:201, 218) */, hipStream_t st);
/* BatchNorm2d + AvgPool2d((4,1)) + permute/reshape to (W, N, C*H) (models.py:241-242, 259-262).  ONE pooled row, from rows 0..3 of z [N][H][W][C];
   rows 4.. lie in no window (dz there = coef[1] z + coef[2]).  All three: C % 8 == 0 and 4 <= H <= 7, else OCRS_ERR_ARG (H >= 8 would have a second
   pooled row); ocrs_avgpool_bn_reduce also needs 256 % (C / 8) == 0.  seq / gseq: fp32 [W][N][C]. */
int ocrs_avgpool_fwd(const void* z, const float* tr, float* seq, int C, int N, int H, int W, int dtype, hipStream_t st);
int ocrs_avgpool_bn_reduce(const float* gseq, const void* z, const float* saved, double* gsum, int C, int N, int H, int W, int dtype, hipStream_t st);
int ocrs_avgpool_dz(const float* gseq, const void* z, const float* coef, void* dz, int C, int N, int H, int W, int dtype, hipStream_t st);
int ocrs_col_sum(const void* a, int ld, int C, float* out, long rows, int dtype, hipStream_t st);
/* nn.GRU(128, 256, bidirectional, 2 layers) recurrence, one layer at a time (models.py:245, 264-266). */
int ocrs_gru_layer_fwd(const float* gi, const float* whh_pk, const float* bhh, float* out, float* saved, int T, int N, hipStream_t st);
int ocrs_gru_layer_bwd(const float* dout, const float* saved, const float* out, const float* whhT_pk, float* dgi, float* dgh, float* dhz, int T,
                       int N, hipStream_t st);
/* The same recurrence as ONE persistent launch per layer and pass (csrc/rec_gru_seq.hip): groups of 16 workgroups own (direction, 32 batch
   columns) and exchange h_t / dgh_t per step with agent-scope 8-byte accesses and an arrival counter.  whh: the fp32 master [2][768][256]
   (weight_hh_l*, weight_hh_l*_reverse stacked; no fragment packing);  sync: ocrs_gru_seq_sync_words(N) 32-bit words (zeroed by the call);
   xws: ocrs_gru_seq_ws_floats(N) floats, the per-step exchange buffer (MFMA-fragment order; initialised by the call);
   err: ONE caller-owned 32-bit word, zeroed once by the caller and sticky -- set if a wait inside a launch timed out (outputs incomplete);
   exact != 0: fp32 MFMA (reference arithmetic), 0: split-bf16 x3 (fp32-class).  ocrs_gru_seq_supported: 1 when every workgroup of the launch
   can be resident on the current device with 64 workgroup slots to spare (otherwise use the per-step entry points above).
   Test hook: with the environment variable OCRS_GRU_SEQ_FAST=0 (read at every launch) every group keeps the agent-scope exchange, also when
   its workgroups share one XCD and would take the L2-local path -- the tests compare the two paths in one process. */
long ocrs_gru_seq_supported(int N);
long ocrs_gru_seq_sync_words(int N);
long ocrs_gru_seq_ws_floats(int N);
int ocrs_gru_seq_fwd(const float* gi, const float* whh, const float* bhh, float* out, float* saved, int T, int N, unsigned* sync, unsigned* err, float* xws,
                     int exact, hipStream_t st);
int ocrs_gru_seq_bwd(const float* dout, const float* saved, const float* out, const float* whh, float* dgi, float* dgh, int T, int N, unsigned* sync,
                     unsigned* err, float* xws, int exact, float* dbih, float* dbhh, hipStream_t st);
/* dbih / dbhh (nullable) [2 * 768]: the bias gradients (column sums of dgi / dgh over time and batch) are ACCUMULATED there by the same launch. */
int ocrs_gru_seq_status(const unsigned* err, hipStream_t st);
/* nn.LogSoftmax(dim=2) (models.py:250). */
int ocrs_log_softmax_fwd(const void* logits, float* out, long rows, int C, int ld, int dtype, hipStream_t st);
int ocrs_log_softmax_bwd(const float* lp, const float* g, void* dlogits, long rows, int C, int ld, int dtype, hipStream_t st);
/* torch.nn.CTCLoss() (ocrs_models/train_rec.py:104,121): forward (alpha) and backward (beta + gradient). */
int ocrs_ctc_fwd(const float* lp, const int* targets, const long long* in_len, const long long* tg_len, float* alpha, float* nll, float* loss,
                 int T, int N, int C, int Lpad, int Smax, hipStream_t st);
int ocrs_ctc_bwd(const float* lp, const int* targets, const long long* in_len, const long long* tg_len, const float* alpha, const float* nll,
                 const float* gout, float* grad, int T, int N, int C, int Lpad, int Smax, hipStream_t st);
/* The same loss with the beta lattice computed by the same launch (alpha and beta recursions side by side, two workgroups per sample) and a
 * backward that is parallel over (sample, time step) -- round 4; loss and gradient bit-identical to ocrs_ctc_fwd + ocrs_ctc_bwd.
 * alpha, beta: workspaces [N][T][Smax] fp32. */
int ocrs_ctc_fwd_ab(const float* lp, const int* targets, const long long* in_len, const long long* tg_len, float* alpha, float* beta, float* nll,
                    float* loss, int T, int N, int C, int Lpad, int Smax, hipStream_t st);
int ocrs_ctc_grad_ab(const float* lp, const int* targets, const long long* in_len, const long long* tg_len, const float* alpha, const float* beta,
                     const float* nll, const float* gout, float* grad, int T, int N, int C, int Lpad, int Smax, hipStream_t st);
/* The same with the alpha lattice kept for the backward in fp16 (BASELINE configs[4] "fp16 CTC alpha/beta"; SURVEY D5: a separately-toleranced
 * variant): alpha16 [N][T][Smax] fp16 = alpha - rowmax, rowmax [N][T] fp32 (row maximum per time step).  The recursion and the loss stay fp32
 * (identical loss bits); the gradient sees the fp16 rounding of the lattice (~1e-3 relative). */
int ocrs_ctc_fwd_h16(const float* lp, const int* targets, const long long* in_len, const long long* tg_len, void* alpha16, float* rowmax, float* nll,
                     float* loss, int T, int N, int C, int Lpad, int Smax, hipStream_t st);
int ocrs_ctc_bwd_h16(const float* lp, const int* targets, const long long* in_len, const long long* tg_len, const void* alpha16, const float* rowmax,
                     const float* nll, const float* gout, float* grad, int T, int N, int C, int Lpad, int Smax, hipStream_t st);
/* preds.argmax(-1) + ctc_greedy_decode_text's collapse (train_rec.py:52; datasets/util.py:147-177). */
int ocrs_ctc_greedy_decode(const float* lp, const long long* in_len, int* amax, int* labels, int* lens, int T, int N, int C, hipStream_t st);
/* levenshtein() of RecognitionAccuracyStats.update (train_rec.py:29-68), unit costs, one row pair per sample: a [N][pa], b [N][pb] int32 label
 * rows, a_len / b_len [N] (clamped to [0, pitch]; entries beyond the length are ignored) -> dist [N] int32.  codes: optional int32[ncodes]
 * class-to-character table (the host compares the characters of decode_text / ctc_greedy_decode_text, datasets/util.py:132-177, and an
 * alphabet with a repeated character makes two ids equal): labels inside the table are compared through it, others as themselves; null
 * (ncodes 0) = identity.  ws: ocrs_edit_distance_ws_bytes(N, pa) bytes.  One launch, no length limit, exact. */
long ocrs_edit_distance_ws_bytes(int N, int pa);
int ocrs_edit_distance(const int* a, const long long* a_len, int pa, const int* b, const long long* b_len, int pb, const int* codes, int ncodes,
                       void* ws, int* dist, int N, hipStream_t st);
/* RecognitionAccuracyStats.update (train_rec.py:29-68; decode_text / ctc_greedy_decode_text, datasets/util.py:132-177) entirely on the device:
 * arg-max + collapse exactly as ocrs_ctc_greedy_decode, targets [N][Lpitch] compacted like decode_text (every entry <= 0 of the whole padded
 * row dropped, tgt_len plays no part), edit distance, then state[0] += sum(dist) (char_errors), state[1] += sum(tgt_len) as given
 * (total_chars).  state: int64[2], accumulated with integer atomics; dist [N] optional (null: not written); codes: optional int32[C] as above.
 * ws: ocrs_ctc_cer_ws_bytes(T, N, Lpitch) bytes (0 = shape not supported).  Two launches, no copy, no synchronisation, no allocation. */
long ocrs_ctc_cer_ws_bytes(int T, int N, int Lpitch);
int ocrs_ctc_cer_update(const float* lp, const long long* in_len, const int* targets, const long long* tgt_len, const int* codes, void* ws,
                        long long* state, int* dist, int T, int N, int C, int Lpitch, hipStream_t st);

/* ------------------------------------------------------------------ input pipeline ----------- */
/* transform_image (ocrs_models/datasets/util.py:27-35): out[i] = float(img_u8[i]) / 255 - 0.5; both pointers 16-byte aligned. */
int ocrs_transform_image_u8(const void* img_u8, void* out, long n, int dtype, hipStream_t st);
/* collate_samples, image part (ocrs_models/train_rec.py:285-299): B crops of H rows, crop b = (H, widths[b]) row-major starting at element
 * offs[b] of `packed` (kind 0: uint8, transform_image fused; kind 1: fp32 already transformed) -> out (B,1,H,Wpad), right-padded with 0.0. */
int ocrs_collate_pad(const void* packed, const long long* offs, const int* widths, void* out, int B, int H, int Wpad, int kind, int dtype,
                     hipStream_t st);
/* torchvision resize(img, [oh, ow], antialias=True) on a float tensor (ocrs_models/datasets/hiertext.py:288-294) =
 * F.interpolate(mode="bilinear", antialias=True, align_corners=False): in [planes][h][w] -> out [planes][oh][ow]; ws = planes*h*ow floats. */
int ocrs_resize_aa(const float* in, float* ws, float* out, int planes, int h, int w, int oh, int ow, hipStream_t st);
long ocrs_resize_aa_ws_floats(int planes, int h, int ow);

/* ------------------------------------------------------------------ training augmentations ---- */
/* The reference's torchvision augmentations (csrc/augment.hip), restated from torchvision's tensor code path for the fixed arguments the
 * training scripts use; parameters are drawn on the host by ocrs_models_amd/augment.py.  params: [B][24] 32-bit words per sample, 16-byte
 * aligned: int kind (0 identity, 1 ColorJitter, 2 nearest affine, 3 perspective, 4 shift (crop / pad), 5 bilinear affine (rotation)),
 * int flags (bit 0: brightness before contrast), int h, w (source), ih, iw (intermediate, after the augmentation), dy, dx (shift: source
 * row / column of intermediate pixel 0), ow (lines: resized width), 7 unused ints, then 8 fp32: jitter {b, c, (float)(1 - c)}; affine
 * {theta row 0 / (w/2), theta row 1 / (h/2), base-grid x and y offsets}; perspective {coeffs 0-2 / (w/2), 3-5 / (h/2), coeffs 6, 7}.
 * The records must describe the packed sources: no kernel reads outside [offs, offs + h * w) of a sample.  Per image h, w <= 65535 and
 * h * w < 2^31 (checked through max_h / max_w).  Contrast means are reduced in a fixed order without atomics: bit-reproducible. */
/* prepare_transform(mask_size, augment) (ocrs_models/train_detection.py:266-290) + default collate: RandomApply(RandomChoice([ColorJitter,
 * RandomAffine, RandomPerspective, RandomCrop(600, pad_if_needed)]), p=0.5) then Resize(mask_size, antialias=False), on the stack
 * [image, mask].  Sample b = uint8 image img_u8 + offs[b] and mask + offs[b] (mask_kind 0: uint8 0/1, 1: fp32), (h, w) row-major;
 * transform_image fused into the load.  img_out (B,1,OH,OW) fp32 / bf16 (dtype 0 / 1), mask_out (B,1,OH,OW) fp32; all 16-byte aligned.
 * ws: ocrs_augment_det_ws_floats(B) floats.  Three launches whatever B. */
long ocrs_augment_det_ws_floats(int B);
int ocrs_augment_det(const void* img_u8, const void* mask, const long long* offs, const int* params, float* ws, void* img_out, float* mask_out,
                     int B, int max_h, int max_w, int OH, int OW, int mask_kind, int dtype, hipStream_t st);
/* The recognition sample path (ocrs_models/datasets/hiertext.py:271-294 with text_recognition_data_augmentations(),
 * datasets/__init__.py:4-30) + collate_samples' image part (train_rec.py:285-299): background masking by the optional uint8 0/1 line masks,
 * RandomApply(RandomChoice([ColorJitter, RandomRotation(5, expand, bilinear, fill -0.5), Pad(5, fill -0.5)]), p=0.5), clamp(-0.5, 0.5)
 * (clamp != 0), antialiased resize to (OH, ow) and right-padding with 0.0 into out (B,1,OH,Wpad) fp32 / bf16.  offs [B][3] = {source element
 * offset of crop and mask, intermediate offset, horizontal-pass offset}; crops kind 0 uint8 (transform fused), 1 fp32.  ws:
 * ocrs_augment_lines_ws_floats(B, inter_floats = sum ih * iw, sum ih * ow) floats.  Five launches whatever B. */
long ocrs_augment_lines_ws_floats(int B, long inter_floats, long hpass_floats);
int ocrs_augment_lines(const void* crops, const void* masks, const long long* offs, const int* params, float* ws, long inter_floats, void* out, int B,
                       int max_ih, int max_iw, int OH, int Wpad, int kind, int clamp, int dtype, hipStream_t st);

/* ------------------------------------------------------------------ validation metrics ------- */
/* Word-level metrics of the detection test() loop (ocrs_models/train_detection.py:177-184) on the device, restating the host contract
 * ocrs_models_amd/postprocess.py (reference postprocess.py:11-36 extract_cc_quads, :102-187 box_match_metrics); csrc/postprocess.hip.
 * Masks are (B, 1, H, W) / (B, H, W): kind 0 = fp32, foreground = value > threshold; kind 1 = uint8 / bool, foreground = non-zero.
 * Components are 8-connected and numbered in raster order of their first pixel (scipy.ndimage.label's order).  Nothing here
 * synchronises the stream: counts stay on the device and every launch is sized from (B, H, W).  ws: caller-owned device memory of the
 * size the matching *_ws_bytes query returns (0 = shape not supported: H or W < 1, or per-image indices beyond 32 bits).
 * ocrs_cc_quads_capacity: the most components an H x W image can hold, ceil(H/2) * ceil(W/2). */
long ocrs_cc_quads_capacity(int H, int W);
long ocrs_cc_quads_ws_bytes(int B, int H, int W);
/* ncomp [B] int; quads [B][capacity][4][2] fp32 (x, y): the min-area rectangle of each component's pixel-centre hull (extract_cc_quads);
 * rows past ncomp[b] are left untouched.  labels (nullable) [B][H][W] int: 0 = background, component id + 1 (scipy.ndimage.label's array). */
int ocrs_cc_quads(const void* mask, int kind, float threshold, int B, int H, int W, int* ncomp, float* quads, int* labels, void* ws,
                  hipStream_t st);
/* box_match_metrics per image: pred_quads [B][cap_p][4][2], target_quads [B][cap_t][4][2] fp32 with device counts n_pred / n_target [B];
 * out [B][4] fp64 = precision | recall | merged_frac | split_frac.  Targets are bucketed by floor(bbox x-min) into nbkt unit-wide
 * columns starting at x = 0 (values outside go to the end buckets; nbkt = 1 compares every pair). */
long ocrs_box_match_ws_bytes(int B, long cap_t, int nbkt);
int ocrs_box_match_metrics(const float* pred_quads, const int* n_pred, long cap_p, const float* target_quads, const int* n_target, long cap_t, int B,
                           int nbkt, double* out, void* ws, hipStream_t st);
/* mask_metrics end to end: ocrs_cc_quads of both batches + ocrs_box_match_metrics; out [B][4] fp64 as above. */
long ocrs_mask_metrics_ws_bytes(int B, int H, int W);
int ocrs_mask_metrics(const void* pred, int pred_kind, const void* target, int target_kind, float threshold, int B, int H, int W, double* out, void* ws,
                      hipStream_t st);

/* ------------------------------------------------------------------ page inference ------------ */
/* From a page to recognition batches (csrc/ocr_infer.hip; Python: ocrs_models_amd/inference/, which states the geometry rules).  Quads are
 * [..][4][2] fp32 (x, y) in pixel-centre coordinates, 16-byte aligned.  Nothing here synchronises: counts are device-side with a capacity.
 *
 * binarize_mask + resize(.., InterpolationMode.NEAREST) (ocrs_models/eval_detection.py:54-57) in one launch: prob (B,1,h,w) fp32 ->
 * out (B,1,H,W) uint8, 1 where prob > threshold; source index min(int(floorf(dst * ((float)in / out))), in - 1) per axis (F.interpolate). */
int ocrs_binarize_resize_nearest(const float* prob, unsigned char* out, int B, int h, int w, int H, int W, float threshold, hipStream_t st);
/* expand_quads (ocrs_models/postprocess.py:39-76; eval_detection.py:67): quads / out [B][cap][4][2]; counts (nullable) [B] int, rows past
 * counts[b] are not written.  Every edge of the rectangle moves outward by dist (centre + axes c0->c1, c1->c2, half-extents + dist; corner k
 * stays corner k); four equal corners are copied; a zero-area ring becomes the rectangle around its segment. */
int ocrs_expand_quads(const float* quads, float* out, const int* counts, int B, long cap, float dist, hipStream_t st);
/* Crop geometry of n = min(*count, cap) quads (count nullable: n = cap), the line-crop step of ocrs_models/datasets/hiertext.py:271-294 applied to
 * word rectangles: plan [cap][8] int = {h, w, ow = line_output_width(h, w, output_height), packed element offset (crops start 16-byte aligned),
 * horizontal-pass element offset (sum of h * ow), first sampler tile, position in (output width, index) order, the quad at this position};
 * totals [805] int64 = {n, packed elements, horizontal-pass elements, sampler tiles, histogram of ow over 0..800}.  One workgroup. */
int ocrs_crop_plan(const float* quads, const int* count, long cap, int output_height, int* plan, long long* totals, hipStream_t st);
/* The crops themselves (hiertext.py:271-283 crops axis-aligned boxes on the host; here rotated rectangles): page (H, W) uint8, transform_image
 * (datasets/util.py:27-35) fused, bilinear, border padding -> packed fp32, crop i (h_i, w_i) row-major at its plan offset.  max_tiles >= totals[3]
 * sizes the launch, packed_floats >= totals[1] bounds the writes. */
int ocrs_rectify_crops(const unsigned char* page, int H, int W, const float* quads, const int* plan, const long long* totals, long max_tiles, float* packed,
                       long packed_floats, hipStream_t st);
/* resize(line_img, [output_height, ow], antialias=True) (hiertext.py:288-294) of every packed crop + collate_samples' right padding with 0.0
 * (train_rec.py:285-299): the crop at position r of the plan's order goes to row r % max_batch of chunk r / max_batch; chunks [nchunks][2] int64 =
 * {element offset in out, Wpad}; pad columns are written too.  Same passes and weights as ocrs_resize_aa: bit-identical to it per crop.
 * ws: ocrs_resize_aa_packed_ws_floats(totals[2]) floats. */
long ocrs_resize_aa_packed_ws_floats(long hpass_floats);
int ocrs_resize_aa_packed(const float* packed, const int* plan, const int* count, long cap, const long long* chunks, int nchunks, int max_batch, float* ws,
                          long ws_floats, float* out, long out_floats, int output_height, hipStream_t st);

/* ------------------------------------------------------------------ text lines ---------------- */
/* Words -> lines in reading order by the geometric rule of DESIGN.md §14 (csrc/text_lines.hip; Python: inference.find_lines; restated in
 * tests/lines_ref.py).  quads [cap][4][2] fp32 as above; n = min(*count, cap) words (count nullable: n = cap); rows, and entries of every
 * output, past n are neither read nor written.  The four stages run in this order on one stream and share ws
 * (ocrs_text_lines_ws_bytes(cap) bytes, 16-byte aligned), which carries the word frames, heads, ranks and line table from one to the next.
 * Nothing synchronises and there are no float atomics: equal input gives equal bytes.
 *
 * ocrs_line_links: word frames, every word's candidate successor with the smallest s (ties: smallest j), acceptance by the chosen word
 * of its nearest chooser (64-bit integer atomicMin of (bits(s) << 32 | k)); next_word [cap] int = the linked successor or -1. */
long ocrs_text_lines_ws_bytes(long cap);
int ocrs_line_links(const float* quads, const int* count, long cap, float max_gap, float min_cos, int* next_word, void* ws, long ws_bytes, hipStream_t st);
/* Head, position in the line and line length of every word by pointer jumping, ceil(log2 cap) rounds: one workgroup in LDS for cap <= 2048,
 * one launch per round above that.  next_word: what ocrs_line_links wrote. */
int ocrs_line_rank(const int* count, long cap, const int* next_word, void* ws, long ws_bytes, hipStream_t st);
/* Lines sorted by their head's (centre y, centre x, word index): n_lines [1] int = L; line_offsets [cap + 1] int, entries 0..L = exclusive scan
 * of the line lengths; word_order [cap] int, the words of line l in chain order at line_offsets[l]; line_of_word [cap] int. */
int ocrs_line_order(const int* count, long cap, int* n_lines, int* line_of_word, int* word_order, int* line_offsets, void* ws, long ws_bytes, hipStream_t st);
/* line_quads [cap][4][2] fp32, rows 0..L-1 (the rest untouched): a one-word line is the word's quad copied; otherwise the rectangle around all
 * corners in the frame u_L = normalise(sum of long side * u over the words in chain order), corners (minU,minV), (maxU,minV), (maxU,maxV), (minU,maxV). */
int ocrs_line_quads(const float* quads, const int* count, long cap, const int* n_lines, const int* line_offsets, const int* word_order, float* line_quads,
                    void* ws, long ws_bytes, hipStream_t st);

/* ------------------------------------------------------------------ page batches -------------- */
/* The page-inference and text-line stages for B pages of different sizes at once (Python: inference.detect_words_batch,
 * find_lines_pages, rectify_crops_pages, ocr_pages).  page_sizes [B][2] int = (H_p, W_p); a page store is the pages' bytes back to back in one
 * uint8 buffer with page_offs [B] int64, the byte offset of each.  ocrs_cc_quads, ocrs_expand_quads, ocrs_crop_plan and ocrs_resize_aa_packed
 * serve batches as they are.  Nothing here synchronises.
 *
 * The masks of all pages in one launch: prob (B,h,w) fp32 -> out (B,Hmax,Wmax) uint8 with Hmax >= H_p, Wmax >= W_p.  Inside (H_p, W_p) the
 * bytes ocrs_binarize_resize_nearest writes for prob[p] and that size alone, 0 outside (written by the same launch).  Padding is background, so
 * ocrs_cc_quads(B, Hmax, Wmax) finds every page's own components in their own raster order. */
int ocrs_binarize_resize_pages(const float* prob, const int* page_sizes, unsigned char* out, int B, int h, int w, int Hmax, int Wmax, float threshold,
                               hipStream_t st);
/* quads [B][cap][4][2] with counts [B] (what ocrs_cc_quads wrote) -> word_offs [B + 1] int = exclusive scan of min(counts, cap); out (nullable)
 * [out_cap][4][2] = the rows of page 0, page 1, ... back to back, each page in its own order, and page_of_word [out_cap] int (rows from out_cap
 * on are dropped).  out == NULL writes word_offs only: the caller reads word_offs[B] to size out, then calls again.  B <= 65535. */
int ocrs_gather_page_quads(const float* quads, const int* counts, int B, long cap, float* out, int* page_of_word, int* word_offs, long out_cap, hipStream_t st);
/* The four text-line stages over the flat words of B pages: page p's words are word_offs[p] .. word_offs[p + 1], n = min(word_offs[B], cap).
 * The rule of §14 with two additions: a word's candidate successors are words of its own page only, and lines are sorted by (page, centre y,
 * centre x, word index) of their head.  The links and order kernels stage only the words of a workgroup's own page (work: sum of n_p^2).
 * Outputs as in "text lines", indices into the flat arrays, plus line_page_offs [B + 1] int (the lines of page p are line_page_offs[p] ..
 * line_page_offs[p + 1]; the last entry is L) and page_of_line [cap] int, rows 0..L-1.  ws: ocrs_text_lines_pages_ws_bytes(cap, B) bytes, 16-byte
 * aligned, shared by the four stages in this order; ocrs_line_rank_pages and ocrs_line_quads_pages are the single-page kernels run on the
 * flat array (links never leave a page).  cap == 0 or B == 0 launches nothing. */
long ocrs_text_lines_pages_ws_bytes(long cap, int B);
int ocrs_line_links_pages(const float* quads, const int* word_offs, int B, long cap, float max_gap, float min_cos, int* next_word, void* ws, long ws_bytes,
                          hipStream_t st);
int ocrs_line_rank_pages(const int* word_offs, int B, long cap, const int* next_word, void* ws, long ws_bytes, hipStream_t st);
int ocrs_line_order_pages(const int* word_offs, int B, long cap, int* n_lines, int* line_of_word, int* word_order, int* line_offsets, int* line_page_offs,
                          int* page_of_line, void* ws, long ws_bytes, hipStream_t st);
int ocrs_line_quads_pages(const float* quads, const int* word_offs, int B, long cap, const int* n_lines, const int* line_offsets, const int* word_order,
                          float* line_quads, void* ws, long ws_bytes, hipStream_t st);
/* ocrs_rectify_crops from a page store: crop i is cut from page page_of_quad[i] (page_of_line for line crops, page_of_word for word crops),
 * whose pointer and size are looked up per workgroup; a page index outside 0..B-1 or a page outside pages_bytes writes nothing.  Same frame,
 * taps and arithmetic: a crop's bytes are those ocrs_rectify_crops writes for it from its own page. */
int ocrs_rectify_crops_pages(const unsigned char* pages, long pages_bytes, const long long* page_offs, const int* page_sizes, int B, const float* quads,
                             const int* page_of_quad, const int* plan, const long long* totals, long max_tiles, float* packed, long packed_floats,
                             hipStream_t st);

/* ------------------------------------------------------------------ tiles --------------------- */
/* Detection in overlapping tiles by the rule of DESIGN.md §20 (csrc/ocr_tiles.hip; Python: inference.tile_plan, tile_batch,
 * binarize_resize_tiles and the tile= argument of the detection drivers; restated in tests/tiles_ref.py).  The reference has no tiled path:
 * both entry points stand where eval_detection.py:32-57 resizes the whole page, with a tile's window in the place of the page.  tiles [T][5]
 * int = {page, y0, x0, th, tw}: window rows y0 .. y0 + th - 1 and columns x0 .. x0 + tw - 1 of that page; the tiles of a page are its tile
 * rows times its tile columns, numbered row-major.  Page store and page_sizes as in "page batches".  Nothing here synchronises.
 *
 * resize(transform_image(page[:, y0:y0+th, x0:x0+tw]), [oh, ow], antialias=True) (eval_detection.py:32-34 on the window alone) for every
 * tile, read from the uint8 store directly: out (T,1,oh,ow) fp32, bit-identical to ocrs_transform_image_u8 + ocrs_resize_aa of the window
 * (the same two passes and weights; the uint8 -> [-0.5, 0.5] map is applied per tap).  Windows may differ in size; max_th >= every th.  Two
 * launches for any T.  A tile that is not inside its page, is taller than max_th, or whose page is not inside pages_bytes is not written.
 * T, max_th, oh <= 65535.  ws: ocrs_tile_batch_ws_floats(T, max_th, ow) floats (host only, no GPU needed; 0 = nothing to do). */
long ocrs_tile_batch_ws_floats(int T, int max_th, int ow);
int ocrs_tile_batch(const unsigned char* pages, long pages_bytes, const long long* page_offs, const int* page_sizes, int B, const int* tiles, int T, int max_th,
                    float* ws, long ws_floats, float* out, int oh, int ow, hipStream_t st);
/* The most tiles a page may have along one axis, and the largest pitch of the cut tables below. */
#define OCRS_TILES_AXIS_MAX 64
/* binarize_mask + resize(.., NEAREST) (eval_detection.py:54-57) of every tile's probabilities into the masks of the pages, one launch:
 * prob (T,h,w) fp32 -> out (B,Hmax,Wmax) uint8, 0 outside (H_p, W_p).  Page p's tiles are tile_offs[p] .. tile_offs[p + 1] - 1 (tile_offs
 * [B + 1] int), grids [B][2] int = (tile rows, tile columns), each in 1 .. max_axis; row_cuts / col_cuts [B][max_axis] int: tile row i owns
 * the page rows after row_cuts[p][i - 1] up to row_cuts[p][i], the last one every row after the cut before it (columns alike).  The byte of
 * page pixel (y, x) is prob[t][ys][xs] > threshold for its owner tile t, ys = min(int(floorf((float)(y - y0) * ((float)h / th))), h - 1) and
 * xs alike: the arithmetic of ocrs_binarize_resize_nearest with the window in the place of the page, so a page with one tile gets the bytes
 * of ocrs_binarize_resize_pages.  1 <= max_axis <= OCRS_TILES_AXIS_MAX, else error 1 and nothing is launched.  A tile index outside 0..T-1
 * contributes background, and source indices are clamped to the tile: a bad table reads nothing outside prob. */
int ocrs_binarize_resize_tiles(const float* prob, int T, int h, int w, const int* tiles, const int* tile_offs, const int* page_sizes, const int* grids,
                               const int* row_cuts, const int* col_cuts, int max_axis, unsigned char* out, int B, int Hmax, int Wmax, float threshold,
                               hipStream_t st);

/* ------------------------------------------------------------------ reading order ------------- */
/* The lines of every page in the order they are read, column by column, and where a new block starts, by the geometric rule of DESIGN.md §16
 * (csrc/reading_order.hip; Python: inference.reading_order; restated in tests/reading_ref.py).  line_quads [cap][4][2] fp32 and n_lines [1] int
 * as ocrs_line_quads / ocrs_line_order wrote them: L = min(*n_lines, cap) lines, in line order.  line_page_offs [B + 1] int as
 * ocrs_line_order_pages wrote it (the lines of page p are line_page_offs[p] .. line_page_offs[p + 1]); NULL with B = 1: one page, lines 0 .. L.
 * Every relation holds between lines of one page only; indices are flat line indices.  The three stages run in this order on one stream and
 * share ws (ocrs_reading_order_ws_bytes(cap, B) bytes, 16-byte aligned; 0 = not supported: cap <= 32768), which carries the line extents from
 * the first to the third.  Nothing synchronises and there are no atomics: equal input gives equal bytes.  cap == 0 or B == 0 launches nothing.
 *
 * ocrs_reading_relation (§16 "Page axis", "Extents", "before"): before [cap][ceil(cap / 32)] uint32, bit (b & 31) of word [a][b >> 5] set iff
 * before(a, b); every word is written, rows and columns from L on and bits between lines of different pages as 0. */
long ocrs_reading_order_ws_bytes(long cap, int B);
int ocrs_reading_relation(const float* line_quads, const int* n_lines, const int* line_page_offs /* NULL = one page */, int B, long cap, unsigned* before,
                          void* ws, long ws_bytes, hipStream_t st);
/* §16 "Order": line_order [cap] int, positions line_page_offs[p] .. line_page_offs[p + 1] = the lines of page p in reading order; one workgroup
 * per page peels the relation: the smallest unemitted line with no unemitted line before it, else (a cycle) the smallest unemitted line.
 * before may be any matrix of that layout; only bits between lines of the same page are read.  Entries from L on are not written. */
int ocrs_reading_peel(const int* n_lines, const int* line_page_offs, int B, long cap, const unsigned* before, int* line_order, void* ws, long ws_bytes,
                      hipStream_t st);
/* §16 "Blocks": new_block [cap] int, 1 where the line at that position of line_order starts a block (always at a page's first position), 0 where
 * rule 1 puts the line before it there and the gap between them is at most block_gap times the taller of the two.  Reads the extents
 * ocrs_reading_relation left in ws.  Entries from L on are not written. */
int ocrs_reading_blocks(const int* n_lines, const int* line_page_offs, int B, long cap, float block_gap, const int* line_order, int* new_block, void* ws,
                        long ws_bytes, hipStream_t st);

/* ------------------------------------------------------------------ characters --------------- */
/* Per-character time spans, page boxes and word ranges of recognised crops by the rule of DESIGN.md §17 (csrc/char_spans.hip; Python:
 * text.greedy_decode_spans, inference.char_boxes / word_chars; restated in tests/chars_ref.py).  The span arrays labels, t0, t1 (int), peak,
 * s0, s1 (fp32) and char_quads ([..][4][2] fp32, 16-byte aligned) have one row per crop at a row pitch of ld entries; the rows of a page are
 * in the crop plan's width-sorted order: row p is the crop of quad plan[p][7].  Entries of a row from lens[row] on are neither read nor
 * written.  Nothing synchronises, there are no atomics: equal input gives equal bytes.  Zero rows launch nothing.
 *
 * ocrs_ctc_greedy_decode that keeps where every character came from (§17 (a)): lp [T][N][C] fp32 log-probs, in_len [N]; sample n writes row
 * row0 + n (ld >= T).  labels and lens are exactly what ocrs_ctc_greedy_decode writes (the arg-max is its arg-max: first maximum on ties);
 * t0 / t1 = first / last time step of the run the character was collapsed from; peak = the largest lp[t][n][label] over the run, a bit copy
 * of that input value.  amax (int), amax_lp (fp32) [N][T]: the arg-max and its value, written on the way (scratch of the caller's).  Two
 * launches; the collapse is one wave per sample, 64 steps per round, any T. */
int ocrs_ctc_decode_spans(const float* lp, const long long* in_len, int* amax, float* amax_lp, int T, int N, int C, long row0, int ld, int* labels, int* t0, int* t1,
                          float* peak, int* lens, hipStream_t st);
/* §17 (b) for the first `rows` rows: quads [cap][4][2] and plan [cap][8] as ocrs_crop_plan read and wrote them.  Character k of row p, crop of
 * quad i = plan[p][7] with ow = plan[i][2]: a0 = clamp(4 t0 - 2, 0, ow), a1 = clamp(4 t1 + 2, 0, ow), s0 = (float)a0 / (float)ow * long side,
 * s1 likewise (positions along the crop's width axis, page pixels); char_quads = P(s0, 0), P(s1, 0), P(s1, short side), P(s0, short side) in
 * the crop frame of quad i (the frame ocrs_rectify_crops samples with).  A row whose plan[p][7] is outside 0..cap-1 is skipped. */
int ocrs_char_boxes(const float* quads, const int* plan, long cap, long rows, int ld, const int* lens, const int* t0, const int* t1, float* s0, float* s1,
                    float* char_quads, hipStream_t st);
/* §17 (c), line crops only: words [wcap][4][2] and the line table (line_quads [cap][4][2], n_lines [1], line_offsets, word_order) as the
 * "text lines" or "page batches" stages wrote them, plan [cap][8] made from line_quads, span rows as above (line l is row plan[l][6]).
 * Word j of a line's chain owns the characters whose centre 0.5f * (s0 + s1) lies in [B_{j-1}, B_j), B_j = the running maximum of
 * 0.5f * (hi_j + lo_{j+1}) over the words' extents along the line's axis; the range then gives up the characters labelled `space` at both
 * ends (space < 0: none).  word_chars [wcap][2] int, indexed by the flat word index: (first, end) into the line's row; an empty range is
 * (e, e).  One wave per line, 64 words per round; entries of words in no line are not written. */
int ocrs_word_chars(const float* words, long wcap, const float* line_quads, const int* n_lines, long cap, const int* line_offsets, const int* word_order,
                    const int* plan, long rows, int ld, const int* labels, const int* lens, const float* s0, const float* s1, int space, int* word_chars,
                    hipStream_t st);

/* ------------------------------------------------------------------ chain crops -------------- */
/* Line crops cut along the polyline of the line's words by the rule of DESIGN.md §21 (csrc/line_chain.hip, the plan in csrc/ocr_infer.hip;
 * Python: inference/chain.py; restated in tests/chain_ref.py), in the place of the line quad's rectangle.  words [wcap][4][2] and the line
 * table (n_lines [1], line_offsets [cap + 1], word_order) as the "text lines" or "page batches" stages wrote them, cap <= wcap.  A line whose
 * offsets do not describe words inside 0..wcap-1 is skipped by every kernel here.  Nothing synchronises, there are no atomics: equal input
 * gives equal bytes.  Zero lines launch nothing.
 *
 * spine [2 wcap][8] fp32, 16-byte aligned: row 2p is the word at chain position p (line l's words are the positions line_offsets[l] ..
 * line_offsets[l + 1] - 1), row 2p + 1 the gap behind it; each {start, len, A.x, A.y, dir.x, dir.y, 0, 0}.  A word's A is the mid-point of its left
 * edge and dir its axis u; a gap leads from the right mid-point of its word to the left one of the next (len 0 and dir 0 where that would go
 * backwards: the spine jumps); the last word of a line has an all-zero gap row.  start = the running fp32 sum of the lengths before, in chain
 * order.  line_dims [cap][2] fp32, 16-byte aligned: S = the sum of all lengths, H = the largest word height.  Rows of lines from n_lines on are
 * not written.  One wave per line, 64 words per round. */
int ocrs_line_spines(const float* words, long wcap, const int* n_lines, long cap, const int* line_offsets, const int* word_order, float* spine, float* line_dims,
                     hipStream_t st);
/* ocrs_crop_plan with (h, w) = (clamp(rint(H), 1, 32768), clamp(rint(S), 1, 32768)) of line_dims in the place of a quad's crop frame: the same
 * kernel, table and totals. */
int ocrs_crop_plan_dims(const float* line_dims, const int* count, long cap, int output_height, int* plan, long long* totals, hipStream_t st);
/* ocrs_rectify_crops along the spine: sample (y, x) of line l's (h, w) crop is the page at P(s, t), s = (x + 0.5) / w * S, t = ((y + 0.5) / h - 0.5) * H,
 * on the last segment of the line with start <= s; the same tiling, clamp and four-tap blend.  plan / totals: ocrs_crop_plan_dims'. */
int ocrs_rectify_chain(const unsigned char* page, int H, int W, const float* spine, const float* line_dims, const int* line_offsets, long wcap, const int* plan,
                       const long long* totals, long max_tiles, float* packed, long packed_floats, hipStream_t st);
/* The same from a page store, as ocrs_rectify_crops_pages: line l is cut from page page_of_line[l]; a crop's bytes are those ocrs_rectify_chain
 * writes for it from its own page. */
int ocrs_rectify_chain_pages(const unsigned char* pages, long pages_bytes, const long long* page_offs, const int* page_sizes, int B, const float* spine,
                             const float* line_dims, const int* line_offsets, long wcap, const int* page_of_line, const int* plan, const long long* totals,
                             long max_tiles, float* packed, long packed_floats, hipStream_t st);
/* ocrs_char_boxes for chain crops, same rows and arrays: s0 = (float)a0 / (float)ow * S, s1 likewise (positions along the spine);
 * char_quads = P(s0, -H/2), P(s1, -H/2), P(s1, +H/2), P(s0, +H/2): a quadrilateral that follows the spine. */
int ocrs_char_boxes_chain(const float* spine, const float* line_dims, const int* line_offsets, long wcap, const int* plan, long cap, long rows, int ld,
                          const int* lens, const int* t0, const int* t1, float* s0, float* s1, float* char_quads, hipStream_t st);
/* ocrs_word_chars for chain crops, same output: word j of a chain owns the characters whose centre 0.5f * (s0 + s1) lies in [b_{j-1}, b_j),
 * b_j = start(word j + 1) - 0.5f * len(gap j) from the spine table (non-decreasing along a chain), less the `space` labels at both ends. */
int ocrs_word_chars_chain(const float* spine, long wcap, const int* n_lines, long cap, const int* line_offsets, const int* word_order, const int* plan, long rows,
                          int ld, const int* labels, const int* lens, const float* s0, const float* s1, int space, int* word_chars, hipStream_t st);

/* ------------------------------------------------------------------ orientation -------------- */
/* Pages scanned sideways or upside down (csrc/page_orient.hip; Python: inference/orient.py; restated for the tests in
 * tests/orient_ref.py).  orientation = k in 0..3: the upright page is rot90(page, k), k quarter turns counter-clockwise.  A point (x, y) of
 * the turned page of a page of H rows and W columns lies on the original page at (x, y) | ((W-1) - y, x) | ((W-1) - x, (H-1) - y) |
 * (y, (H-1) - x) for k = 0 | 1 | 2 | 3 (pixel centres).  Nothing here allocates or synchronises.
 * ocrs_turn_page_u8: dst = rot90(src, k) for the (H,W) uint8 page src, k in 1..3 (k = 0 is the caller's own page); dst is (W,H) for odd k and
 * must not overlap src.  Any H, W >= 1. */
int ocrs_turn_page_u8(const unsigned char* src, int H, int W, int k, unsigned char* dst, hipStream_t st);
/* The table above (inverse == 0: turned-page points -> original-page points) or its inverse (original -> turned) on quads [n][4][2] fp32 of
 * a page whose ORIGINAL is H x W: one fp32 operation per coordinate, corner j -> corner j.  count: optional device int32, only the first
 * min(count, n) rows are written. */
int ocrs_turn_quads(const float* quads, long n, const int* count, int H, int W, int k, int inverse, float* out, hipStream_t st);
/* The axis vote.  Per quad the long side L and the short side by the crop-frame rule (the longer of c0->c1 and c1->c2; on a tie the one with
 * the larger |x|), lengths as sqrtf(x * x + y * y) with one rounding per operation; a quad votes if short > 0 and long >= min_aspect * short
 * (fp32) and adds |L| to H if |L.x| >= |L.y|, else to V.  votes: 2 fp64 (H, V) followed by 2 int32 (voters, K = min(sample, voters)), 24
 * bytes, 8-byte aligned; the sums have a fixed order (no atomics).  picks [sample] int32: the K voters with the largest |L|, ties by the
 * smaller index, in that order; entries from K on are -1.  count as above. */
int ocrs_orient_votes(const float* quads, long n, const int* count, float min_aspect, int sample, double* votes, int* picks, hipStream_t st);
/* scores[r] (fp64) = the mean over t < steps[r] of max_c log_probs[t][r][c] for the [T][B][C] fp32 log-probs of B crops, 1 <= steps[r] <= T
 * (clamped; 0 steps give 0): the maxima exact, the sum in time order in fp64. */
int ocrs_path_confidence(const float* log_probs, int T, int B, int C, const int* steps, double* scores, hipStream_t st);

/* ------------------------------------------------------------------ directions --------------- */
/* Text in mixed directions on one page (csrc/line_dirs.hip; Python: inference/directions.py; restated for the tests in
 * tests/directions_ref.py): the sideways words of a page are read as the words of a second, virtual page, the page turned by one quarter
 * turn, through the page-batch path.  Nothing here allocates or synchronises.
 * ocrs_axis_split: per quad of quads [n][4][2] fp32 the long side L by the crop-frame rule (the longer of c0->c1 and c1->c2; on a tie the one
 * with the larger |x|; lengths as sqrtf(x * x + y * y), one rounding per operation); the quad is SIDEWAYS iff none of its eight coordinates is
 * a NaN and |L.y| > |L.x|.  With m = min(count, n) rows (count: optional device int32) of which U are upright: out_quads rows 0 .. U - 1 are
 * the upright quads as they are, rows U .. m - 1 the sideways quads mapped to the page turned by one quarter turn, (x, y) -> (y, (W-1) - x),
 * the bits ocrs_turn_quads(k = 1, inverse = 1) gives; both groups in input order (a scan, no atomic counter: equal input gives equal
 * bytes).  page_of_word [n] = 0 | 1, source_index [n] = the input row of every output row, word_offs [3] = 0, U, m.  Rows from m on are not
 * written.  16-byte aligned quads and out_quads, which must not overlap.  n == 0 launches nothing (word_offs is then the caller's).  n <= 65536:
 * the call has no workspace, so every workgroup of 256 rows classifies all rows again -- sized for the words of one page (a few thousand);
 * more is error 1. */
int ocrs_axis_split(const float* quads, long n, const int* count, int H, int W, float* out_quads, int* page_of_word, int* word_offs, int* source_index,
                    hipStream_t st);
/* batch_out = batch_in, an [n][OH][Wpad] fp32 recognition batch, with every crop i whose flags[i] != 0 (flags NULL: every crop) turned by 180
 * degrees within its valid width w = clamp(widths[i], 0, Wpad): out[i][y][x] = in[i][OH - 1 - y][w - 1 - x] for x < w; the columns from w on
 * and the other crops are copied.  An exact permutation of the 4-byte elements.  Any Wpad >= 1 and any 4-byte aligned bases; where Wpad is a
 * multiple of 4 and batch_out is 16-byte aligned a lane moves 16 bytes, reversed in registers.  batch_out must not overlap batch_in. */
int ocrs_flip_crops(const float* batch_in, float* batch_out, long n, int OH, int Wpad, const long long* widths, const int* flags, hipStream_t st);
/* flags[i] = (probe[i] != 0 && s_flip[i] > s_plain[i]) ? 1 : 0 for n crops: the comparison in fp64 and strict, so equal scores and a NaN on
 * either side give 0; probe is the page of every crop's line (0 = upright, never flipped) or any int32 mask. */
int ocrs_flip_flags(const double* s_plain, const double* s_flip, const int* probe, long n, int* flags, hipStream_t st);

/* ------------------------------------------------------------------ beam search -------------- */
/* CTC prefix beam search and forced alignment by the rule of DESIGN.md §18 (csrc/ctc_beam.hip; Python: text.beam_decode_spans,
 * text.ctc_align_spans; restated in tests/beam_ref.py).  Both generalise ctc_greedy_decode_text (datasets/util.py:147-177), the greedy rule:
 * it returns the labelling of the single most probable alignment, the beam the most probable labelling among the prefixes it kept.  lp
 * [T][N][C] fp32 log-probs, class 0 = blank, in_len [N] (clamped to 0..T); sample n reads / writes row row0 + n of the span arrays (pitch
 * ld >= T), as ocrs_ctc_decode_spans does.  One launch each, nothing synchronises, integer LDS atomics only: equal input gives equal bytes.
 *
 * Workspace sizes (host only, no GPU needed; 0 = shape not supported).  Beam: the prefix tree, (T W + 1) nodes of 8 bytes per sample.
 * Align: two 64-bit back-pointer words per step and 64 states, for labellings of up to min(Lmax, T) labels. */
long ocrs_ctc_beam_ws_bytes(int T, int N, int W);
long ocrs_ctc_align_ws_bytes(int T, int N, int Lmax);
/* Stands in for ctc_greedy_decode_text (datasets/util.py:147-177) with a beam of W prefixes, 1 <= W <= 64, 2 <= C <= 256 (anything else:
 * error 1, nothing launched).  Per step every prefix stays (blank, a repeat of its last label, and the mass of its parent prefix extending
 * into it) and extends by every label 1..C-1; the W largest totals survive, ties by (slot, stay before extend, label) ascending; no label
 * pruning.  labels / lens: the labelling of the best prefix after the last step; score [rows] fp32: its log-mass (in_len 0: empty, 0.0; no
 * candidate of finite mass left: empty, -inf).  Entries of a row from lens on are not written.  ws: 8-byte aligned,
 * ocrs_ctc_beam_ws_bytes(T, N, W) bytes.  One workgroup per sample. */
int ocrs_ctc_beam_decode(const float* lp, const long long* in_len, int T, int N, int C, int W, long row0, int ld, int* labels, int* lens, float* score, void* ws,
                         long ws_bytes, hipStream_t st);
/* ocrs_ctc_beam_decode with a character n-gram language model fused into the ranking (Python: text.CharLM, lm= of
 * text.beam_decode_spans; restated in tests/beam_lm_ref.py; no reference counterpart).  gain: dense fp32 table of C^order entries, order in
 * 1..3; gain[ctx..., c] is the credit for appending label c after the last order - 1 labels of the prefix (padded on the left with 0, the
 * blank, which never occurs inside a labelling); entries finite or -inf (a forbidden transition), column c = 0 never read.  Every prefix
 * carries lm, the fp32 sum of its labels' gains in order; candidates are ranked by total + lm and exist iff total and rank are both > -inf;
 * the CTC numbers, merges and tie rule are those of ocrs_ctc_beam_decode, and a table of zeros gives its bytes.  score: the CTC log-mass of
 * the best prefix's labelling, as above; lm_score [rows] fp32: its lm (in_len 0 and nothing survived: 0).  Argument checks and workspace as
 * ocrs_ctc_beam_decode, plus gain and lm_score not NULL and order in 1..3 (else error 1, nothing launched). */
int ocrs_ctc_beam_decode_lm(const float* lp, const long long* in_len, int T, int N, int C, int W, const float* gain, int order, long row0, int ld, int* labels,
                            int* lens, float* score, float* lm_score, void* ws, long ws_bytes, hipStream_t st);
/* The t0 / t1 / peak that ocrs_ctc_decode_spans derives from ctc_greedy_decode_text's runs (datasets/util.py:147-177), for a GIVEN labelling:
 * Viterbi over blank | l1 | blank | ... | lL | blank (ties: stay, then one state back, then two; the final blank wins a tied end).  Reads
 * labels / lens of rows row0 .. row0 + N - 1; character k gets the first / last step the path spends in its state and peak = the largest
 * lp[t][n][l_k] over them, a bit copy.  lens = -1 where no alignment has a finite score (more labels than steps, no room for the blank between
 * equal neighbours, a label outside 1..C-1, more labels than ws was sized for, or more than 3199); rows with lens < 0 are skipped.  ws:
 * 8-byte aligned, at least the size for Lmax = 0.  One wave per sample. */
int ocrs_ctc_align_spans(const float* lp, const long long* in_len, int T, int N, int C, long row0, int ld, const int* labels, int* lens, int* t0, int* t1,
                         float* peak, void* ws, long ws_bytes, hipStream_t st);

/* ------------------------------------------------------------------ end-to-end accuracy ------- */
/* Page OCR scored against annotated words by the rule of DESIGN.md §23 (csrc/ocr_eval.hip; Python: inference/evaluate.py; restated for the
 * tests in tests/eval_ref.py).  Everything is pooled over the B pages of a call: pred_quads [P][4][2] and gt_quads [G][4][2] fp32 (convex
 * quads), page b owning rows pred_offs[b] .. pred_offs[b + 1] resp. gt_offs[b] .. gt_offs[b + 1] (both [B + 1] int); gt_ignore [G] bytes
 * (non-zero = "do not care").  pair_offs [B + 1] int64: the dense (predictions x annotations) IoU matrix of page b, row-major, starts at
 * element pair_offs[b] of iou [n_pairs] fp64; max_pairs = the largest matrix of the call (it sizes the grid).  The host knows every one of
 * these numbers from its inputs: nothing synchronises and nothing is allocated, and a dense matrix has no capacity that could overflow.  A page
 * whose offsets do not describe rows inside the arrays is skipped by every kernel.  B <= 65535.  Only integers are accumulated: equal input
 * gives equal bytes.
 *
 * ocrs_eval_pair_iou: every element of every page's matrix is written: 0.0 where the strict bounding-box test of box_match_metrics fails,
 * either area is zero or the intersection is not positive, else inter / (pa + ga - inter) with quad_inter and area_of of the validation metrics
 * (bit for bit the host's quad_intersection_area / _area arithmetic).  ign_hit [P] int: zeroed, then 1 where inter / pa > 0.5 against an
 * ignored annotation of the prediction's page. */
int ocrs_eval_pair_iou(const float* pred_quads, const int* pred_offs, const float* gt_quads, const int* gt_offs, const unsigned char* gt_ignore,
                       const long long* pair_offs, int B, long P, long G, long n_pairs, long max_pairs, double* iou, int* ign_hit, hipStream_t st);
/* The greedy one-to-one matching of each page: candidates are the pairs with a not ignored annotation and iou > min_iou, totally ordered by
 * (iou descending, prediction ascending, annotation ascending); a pair is taken when both its ends are free.  One workgroup per page, rounds
 * of mutually-best pairs (exactly the greedy result, since the order is strict).  gt_of_pred [P] int: the annotation's index WITHIN ITS PAGE,
 * -1 = unmatched, -2 = unmatched and ign_hit set (ignored); pred_of_gt [G] int likewise (-1 = unmatched); iou_of_pred [P] fp64: the matched
 * pair's IoU, 0.0 otherwise.  ws: ocrs_eval_match_ws_bytes(P, G) bytes, 4-byte aligned. */
long ocrs_eval_match_ws_bytes(long P, long G);
int ocrs_eval_match(const double* iou, const long long* pair_offs, const int* pred_offs, const int* gt_offs, const unsigned char* gt_ignore,
                    const int* ign_hit, int B, long P, long G, long n_pairs, double min_iou, int* gt_of_pred, int* pred_of_gt, double* iou_of_pred, void* ws,
                    hipStream_t st);
/* Texts are Unicode code points: pred_text [n_pred_text] int with pred_text_offs [P + 1] int, gt_text / gt_text_offs [G + 1] likewise.  For
 * every prediction: dist [P] int = the Levenshtein distance to its matched annotation (the wave routine of ocrs_edit_distance, no code table),
 * -1 when unmatched; flags [P] int = 1 (equal) | 2 (equal after folding ASCII A-Z to lower case only), 0 when unmatched.  bnd: n_pred_text
 * ints of scratch.  max_page_preds = the largest number of predictions on one page (it sizes the grid).  state (NULL = no counting): int64
 * [12], integer atomics ADD to it across calls: pages | predictions not ignored | annotations not ignored | predictions ignored | matched
 * pairs | exact | exact ignoring ASCII case | edit distance over matched pairs | annotated characters of matched pairs | predicted characters
 * of unmatched, not ignored predictions | annotated characters of unmatched, not ignored annotations | annotated characters of all not ignored
 * annotations.  Two launches. */
int ocrs_eval_text_update(const int* pred_offs, const int* gt_offs, const unsigned char* gt_ignore, int B, long P, long G, int max_page_preds,
                          const int* gt_of_pred, const int* pred_of_gt, const int* pred_text, const int* pred_text_offs, long n_pred_text,
                          const int* gt_text, const int* gt_text_offs, long n_gt_text, int* bnd, int* dist, int* flags, long long* state, hipStream_t st);

/* ------------------------------------------------------------------ layout model -------------- */
/* LayoutModel (ocrs_models/models.py:340-406) and its loss / statistics (train_layout.py:15-171); csrc/layout.hip.  All storage fp32; a row is
 * one (page n, word w) token, row index n * W + w.  The Linear layers run on ocrs_conv_igemm / ocrs_gemm_x3[p] / ocrs_wgrad_*.
 * Dropout (the four sites of nn.TransformerEncoderLayer, torch/nn/modules/transformer.py as instantiated at models.py:385-388): p = 0 skips it;
 * otherwise element i of a site's tensor is kept iff word (i & 3) of Philox-4x32-10(counter = (i >> 2, site), key = seed) >= p * 2^32, and kept
 * values are scaled by 1 / (1 - p).  `site` = 4 * layer + {0 attention probabilities, 1 after out_proj, 2 after the ReLU, 3 after linear2}.
 * Masks are regenerated by the backward entry points from the same (p, seed, site); ocrs_layout_dropout_mask writes one out (1 = kept). */
int ocrs_layout_dropout_mask(unsigned char* mask, long n, float p, long seed, int site, hipStream_t st);
/* SinPositionalEncoding(256) (models.py:271-337): boxes [rows][4] -> out [rows][256]; rates [32] = 1 / 10000^(j / 32) as the reference's fp32
 * expression yields them.  Coordinates are rounded half to even; they must be >= 0 and < 2^24. */
int ocrs_layout_embed(const float* boxes, const float* rates, float* out, long rows, hipStream_t st);
/* Self-attention of nn.TransformerEncoderLayer(256, 4) with batch_first=False (models.py:385-388, 400): qkv [S][W][768] = the in-projection's
 * output (q | k | v, 4 heads of 64), the SEQUENCE axis is the leading one (the pages of the batch), W the independent batch axis; out [S][W][256]
 * = dropout(softmax(q k^T / 8)) v per (w, head), the layout out_proj reads.  Exact-fp32 MFMA.  1 <= S <= 128 (ocrs_layout_attn_supported).
 * The dropout element index is ((w * 4 + head) * S + query) * S + key.
 * _bwd: dout [S][W][256] -> dqkv [S][W][768] (every element written), probabilities and masks recomputed. */
long ocrs_layout_attn_supported(int S); /* 1 / 0 */
int ocrs_layout_attn_fwd(const float* qkv, float* out, int S, int W, float p, long seed, int site, hipStream_t st);
int ocrs_layout_attn_bwd(const float* qkv, const float* dout, float* dqkv, int S, int W, float p, long seed, int site, hipStream_t st);
/* y = LayerNorm(x + dropout(a)) over rows of 256 (norm1 / norm2 with dropout1 / dropout2 of the post-norm encoder layer, models.py:385-388);
 * stat (nullable) [rows][2] = mean | rstd for the backward. */
int ocrs_layout_ln_fwd(const float* x, const float* a, const float* gamma, const float* beta, float* y, float* stat, long rows, float eps, float p, long seed,
                       int site, hipStream_t st);
/* Its backward: dy = dy1 (+ dy2, nullable: the two gradient paths into a layer output are summed on load); ds [rows][256] = dL/d(x + dropout(a))
 * (the residual branch's gradient; with p = 0 also the gradient of a); da (p > 0) = the gradient of a.  dgamma / dbeta [256] are WRITTEN as
 * fixed-order sums of per-workgroup partials in ws (ocrs_layout_ln_bwd_ws_floats(rows) floats). */
long ocrs_layout_ln_bwd_ws_floats(long rows);
int ocrs_layout_ln_bwd(const float* dy1, const float* dy2, const float* x, const float* a, const float* stat, const float* gamma, float* ds, float* da,
                       float* dgamma, float* dbeta, float* ws, long rows, float p, long seed, int site, hipStream_t st);
/* dropout(relu(.)) on the feed-forward hidden [n] in place (models.py:385-388: activation + dropout of the encoder layer); relu = 0 when the
 * producing GEMM already applied it.  _bwd: out = g / (1 - p) where the stored h > 0, else 0 (out may alias g). */
int ocrs_layout_relu_drop_fwd(float* h, long n, int relu, float p, long seed, int site, hipStream_t st);
int ocrs_layout_relu_drop_bwd(const float* g, const float* h, float* out, long n, float p, hipStream_t st);
/* Bias gradients of the Linear layers (autograd of models.py:388, 390): out[c] = sum over rows of a[row][c], c < Cout <= C (C % 4 == 0 columns
 * are read), WRITTEN as a fixed-order sum of per-workgroup partials in ws (ocrs_layout_col_sum_ws_floats(C, rows) floats). */
long ocrs_layout_col_sum_ws_floats(int C, long rows);
int ocrs_layout_col_sum(const float* a, int ld, int C, int Cout, float* out, float* ws, long rows, hipStream_t st);
/* classify's padded output [rows][ld] -> [rows][2], through the sigmoid when probs != 0 (models.py:401-406); and the reverse for its gradient:
 * g [rows][2] -> dlog [rows][ld] with zero padding columns. */
int ocrs_layout_head_out(const float* logits, int ld, float* out, long rows, int probs, hipStream_t st);
int ocrs_layout_head_grad_in(const float* g, float* dlog, int ld, long rows, hipStream_t st);
/* weighted_loss() = BCEWithLogitsLoss(pos_weight) with mean reduction over rows * 2 elements (train_layout.py:94-97, 128, 166) in one launch:
 * loss [1]; dlogits (nullable) [rows][2] = d loss / d pred; counts (nullable) [6] int64 = per class {true positives, predicted positives,
 * target positives} of LayoutAccuracyStats.update (train_layout.py:46-58), a prediction being positive when sigmoid(pred) >= 0.5 in fp32
 * (train_layout.py:131), or pred >= 0.5 when pred_is_prob != 0 (test(), train_layout.py:164-167, which also feeds the probabilities to the
 * logits loss).  ws: ocrs_layout_loss_ws_bytes() bytes whose first word is zero on entry (and left zero). */
long ocrs_layout_loss_ws_bytes(void);
int ocrs_layout_loss(const float* pred, const float* target, float pos_weight, int pred_is_prob, float* loss, float* dlogits, long long* counts, void* ws,
                     long rows, hipStream_t st);
/* precision_recall of both classes (train_layout.py:24-35, 55-63: int64 counts divided as fp32, 0 / 0 = NaN) added to the running sums on the
 * device: sums [5] fp64 = line-start precision | recall | line-end precision | recall | number of updates. */
int ocrs_layout_stats_update(const long long* counts, double* sums, hipStream_t st);
/* One batch of WebLayout.__getitem__ + F.pad + default_collate (ocrs_models/datasets/web_layout.py:76-186; csrc/layout_data.hip) from the
 * dataset parsed once into device memory: coords [T][4] fp64 (left, top, right, bottom of every word, pages back to back in paragraph ->
 * word order), para [T] = the paragraph index of a word within its page, page_off [P + 1] = first word of a page, viewport [P][2] =
 * int(width), int(height).  pages [N] in 0 .. P-1, jitter [N][2] fp64 (x, y; web_layout.py:92-95) -> boxes [N][W][4], labels [N][W][2] fp32
 * (line_start, line_end).  Per coordinate c * 1.0 + jitter, then c / viewport - 0.5 if normalize != 0, each a single fp64 operation, rounded
 * to fp32 once (torch.Tensor(words), web_layout.py:174).  A label is set when the word has no previous / next word in its paragraph or
 * intervals_overlap (datasets/util.py:197-204) of the two transformed vertical intervals is false; the neighbour of slot W - 1 is word W of
 * the page (web_layout.py:177-184 truncates after labelling).  Slots past the page's word count are 0.0.  Every element is written. */
int ocrs_weblayout_batch(const double* coords, const int* para, const long long* page_off, const double* viewport, int P, const int* pages,
                         const double* jitter, int N, int W, int normalize, float* boxes, float* labels, hipStream_t st);
/* Recognition training data (csrc/line_data.hip; Python: ocrs_models_amd/datasets.py HierTextRecognition / DeviceLineLoader).
 * ocrs_line_mask: generate_mask(w, h, [poly], shrink_dist=0.0) of ocrs_models/datasets/util.py:78-110 as called by hiertext.py:262, i.e. PIL's
 * ImageDraw.polygon(poly, fill="white", outline=None) on a mode "1" image, bit for bit, for n polygons in one launch.  vertices [..][2] int32
 * (x, y), polygon i = vertex_counts[i] (2 .. 512) vertices from vertex_offs[i], coordinates within +-65535 (the host checks both); sizes [n][2] int32 (h, w) of its canvas; its 0/1 byte mask
 * (h * w, row-major) is written at out_u8 + out_offs[i].  max_h >= every h (it sizes the grid).  Self-intersecting polygons get whatever the
 * restated scanline rules give (tests/hiertext_ref.py), and so do polygons that pass twice through one vertex; parity with PIL (12.2.0) is
 * pinned for simple polygons only (DESIGN.md section 12 says on how many). */
int ocrs_line_mask(const int* vertices, const long long* vertex_offs, const int* vertex_counts, const int* sizes, const long long* out_offs,
                   void* out_u8, int n, int max_h, hipStream_t st);
/* One batch of HierTextRecognition._get_line_image + generate_mask (hiertext.py:256-263) from the line store in device memory: pixels_u8 = the
 * un-resized grey crops back to back, line l = sizes[l] (h, w) bytes from pixel_offs[l], its polygon as above (vertices relative to the crop's
 * origin); N lines.  For b < B, line indices[b] (0 .. N-1) is copied to out_crops_u8 + batch_offs[3 * b] and its mask rasterised at
 * out_masks_u8 + batch_offs[3 * b]: batch_offs is the [B][3] offset table of ocrs_augment_lines, which runs next on these two buffers.
 * max_h >= the height of every line of the batch. */
int ocrs_line_batch(const void* pixels_u8, const long long* pixel_offs, const int* sizes, const int* vertices, const long long* vertex_offs,
                    const int* vertex_counts, int N, const int* indices, int B, int max_h, const long long* batch_offs, void* out_crops_u8,
                    void* out_masks_u8, hipStream_t st);

/* ------------------------------------------------------------------ detection page store ------ */
/* Detection training data (csrc/page_data.hip; Python: ocrs_models_amd/datasets.py HierText / DDI100 / DevicePageLoader).
 * ocrs_shrink_polygons: shrink_polygon(poly, dist) of ocrs_models/datasets/util.py:54-75 as generate_mask calls it (util.py:96-102), for n
 * polygons in one launch, one thread each, by the project's own rule (the mitred inward offset with GEOS' mitre limit
 * of 5, a ring that would split or flip is skipped; tests/detdata_ref.py states it operation by operation).  vertices [..][2] int32 (x, y),
 * polygon i = vertex_counts[i] (<= 512) vertices from vertex_offs[i], coordinates within +-65535 (the host checks both).  Polygon i's result
 * starts at element 2 * vertex_offs[i] of out_xy [..][2] fp64 (the shrunk ring) and of out_vertices [..][2] int32 (the same truncated as PIL
 * converts float polygon coordinates: towards zero); both hold 2 * (all vertices) points.  out_counts [n] = its vertex count, 0 = skipped,
 * -1 = more than 512; out_rows [n][2] = the first and last row its fill can touch (y_min, y_max of out_vertices; 0, -1 when skipped).
 * ws: 3 * (all vertices) ints.  dist == 0.0 copies the vertices (generate_mask's bypass, util.py:97-100). */
int ocrs_shrink_polygons(const int* vertices, const long long* vertex_offs, const int* vertex_counts, int n, double dist, int* ws, double* out_xy,
                         int* out_vertices, int* out_counts, int* out_rows, hipStream_t st);
/* One batch of HierText.__getitem__ / DDI100.__getitem__ up to the transform (hiertext.py:73-92, ddi100.py:77-94) from the page store in
 * device memory: pixels_u8 = the grey pages back to back, page l = sizes[l] (h, w) bytes from pixel_offs[l]; N pages.  For b < B, page
 * indices[b] (0 .. N-1) is copied to out_pages_u8 + batch_offs[b] and generate_mask(w, h, its polygons) (util.py:78-110: the union of PIL's
 * ImageDraw.polygon(fill, outline=None) over the shrunk polygons, each by ocrs_line_mask's rules) is written as 0/1 bytes at out_masks_u8 +
 * batch_offs[b]: batch_offs is the offset table of ocrs_augment_det, which runs next on these two buffers.  polys [n_polys][4] int32 = {first
 * vertex in vertices, vertex count (0 = skipped), y_min, y_max} with each page's polygons sorted by y_min; bands [..][2] int32 = the slice
 * [lo, hi) of polys that can touch a band of 16 rows, page l's ceil(h / 16) bands starting at band_offs[l].  Pixel, batch and output offsets
 * that are multiples of 16 move 16 bytes per lane.  max_h / max_w >= the height / width of every page of the batch. */
int ocrs_page_batch(const void* pixels_u8, const long long* pixel_offs, const int* sizes, const int* vertices, long n_vertices, const int* polys,
                    int n_polys, const long long* band_offs, const int* bands, int N, const int* indices, int B, int max_h, int max_w,
                    const long long* batch_offs, void* out_pages_u8, void* out_masks_u8, hipStream_t st);

/* ------------------------------------------------------------------ optimiser ---------------- */
/* table [nt][5] int64 {param, grad, exp_avg, exp_avg_sq, numel}; chunks [nchunks][2] int32 {tensor, chunk of ocrs_opt_chunk()}. */
int ocrs_opt_chunk(void);
/* torch.nn.utils.clip_grad_norm_ (ocrs_models/train_rec.py:148). */
int ocrs_clip_grad_norm(const long long* table, const int* chunks, int nchunks, float max_norm, double* sumsq, float* norm_out,
                        float* coef_out, int scale_in_place, hipStream_t st);
/* torch.optim.Adam.step (ocrs_models/train_detection.py:97,378; train_rec.py:151,381). */
int ocrs_adam_step(const long long* table, const int* chunks, int nchunks, float b1, float b2, float eps, float step_size, float bc2_sqrt,
                   const float* gscale, hipStream_t st);
/* The same step in capturable form (a train step recorded into a hipGraph, ocrs_models_amd/graph.py): the step count is a device fp32 [1]
   (incremented by this call before use), bias corrections are derived on the device; lr is the only per-step host scalar. */
int ocrs_adam_step_dev(const long long* table, const int* chunks, int nchunks, double b1, double b2, float eps, double lr, float* step,
                       const float* gscale, hipStream_t st);
int ocrs_fill_f32(float* p, float v, long n, hipStream_t st);

/* Measurement support (csrc/prof.hip): while enabled, every launch of the DepthwiseConv block-backward families records its start / stop timestamps
   from the dispatch packet itself (hipExtLaunchKernelGGL) -- no event barrier packets between the kernels.  ocrs_prof_count: launches recorded
   so far;  ocrs_prof_read: durations in ms of launches [first, first + n) into a HOST array (synchronises the stream). */
int ocrs_prof_enable(int on);
long ocrs_prof_count(void);
int ocrs_prof_read(float* ms, long first, long n, hipStream_t st);
/* Test support for the data-parallel path (reference: none -- train_detection.py:375-376 is single-process): `blocks` 256-thread
   workgroups that stay resident for `micros` microseconds on stream st, the CU footprint of a collective's channel kernels.  The persistent
   GRU launches must survive next to it (tests/test_train_loop_gpu.py::test_persistent_gru_under_rccl_allreduce_load). */
int ocrs_cu_hog(int blocks, int micros, hipStream_t st);

#ifdef __cplusplus
}
#endif
#endif /* OCRS_HIP_H */
