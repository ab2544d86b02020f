// Host-side internals the detection files share (C++ linkage; the C ABI is include/ocrs_hip.h).  Included by the file that defines each function
// and by every file that calls it, so a prototype that drifts from its definition fails to compile or link.  `*_supported` = 1 / true: the
// kernel takes that call; the caller then uses `*_launch` (and sizes its workspace with `*_ws_floats` / `*_gx` / `*_blocks`).
#pragma once
#include "det_common.h"

// det_bwd.hip: dw[(e / cin) * ldw + e % cin] += sum_b ws[b][e] (k_wgrad_partials_reduce), queued instead while a deferral window is open
// (may_defer = false: launched now in any case -- for a workspace that the next launch overwrites)
void det_wgrad_reduce_launch(const float* ws, int nb, int nelem, float* dw, int cin, int ldw, hipStream_t st, bool may_defer = true);

// det_c1.hip: the first block's row-pair kernels.  supported: whole 64-column segments and row pairs (W % 64 == 0, H % 2 == 0)
long det_c1v2_supported(int N, int H, int W);
int det_c1v2_bwd_launch(const float* img, const float* wdw, const float* wpw, const void* g, const void* z, const float* bn, const float* coef,
                        double* acc64, int N, int H, int W, int dtype, hipStream_t st);
// det_pw2.hip: pointwise backward k_pw_bwd2.  supported: bf16, one K chunk, Cin and Cout in {8, 16, 32} (Cout <= 32)
long det_pw2_supported(int Cin, int Cout, int dtype);
long det_pw2_ws_floats(int Cin, int Cout, int N, int H, int W);
int det_pw2_launch(const void* xa, const void* xb, int Ca, int Cb, const float* tra, const float* trb, const float* wdw, const void* g1, const void* g2,
                   int pooled, const void* z, const float* bn, const float* coef, const void* wpk_d, void* du, float* dwpw, float* ws, int Cout, int N,
                   int H, int W, int ldu, int ldw, hipStream_t st, bool may_defer = true);
// det_pwb.hip: deep-level pointwise backward k_pwb.  supported: bf16, Cin in {32 .. 256}, Cout in {64, 128, 256} (Cout >= 64), Cin * 8 >= Cout
long det_pwb_supported(int Cin, int Cout, int dtype);
int det_pwb_gx(int Cin, int Cout, int N, int H, int W, int pooled);  // blocks of the launch = workspace slots of Cin * Cout floats
int det_pwb_launch(const void* xa, const void* xb, int Ca, int Cb, const float* tra, const float* trb, const float* wdw, const void* g1, const void* g2,
                   int pooled, const void* z, const float* bn, const float* coef, const void* wpk_d, void* du, float* dwpw, float* ws, int Cout, int N,
                   int H, int W, const BnFin* fin, hipStream_t st);
// det_dwf.hip: deep-level block forward k_dwf (no fused max-pool).  supported: bf16, the shapes of det_pwb_supported
long det_dwf_supported(int Cin, int Cout, int dtype);
int det_dwf_launch(const void* xa, const void* xb, int Ca, int Cb, const float* tra, const float* trb, const float* wdw, const void* wpk, void* z,
                   double* gstat, int Cout, int N, int H, int W, hipStream_t st, const FwdFin& fin);
// det_ctf.hip: deep-level ConvTranspose forward k_ctf.  supported: bf16, (Cup, Cout) in {(256, 128), (128, 64), (64, 32)}
long det_ctf_supported(int Cup, int Cout, int dtype);
int det_ctf_launch(const void* x, const float* tr, const void* wpk, const float* bias, void* out, int Cup, int Cout, int N, int h, int w, int H, int W,
                   hipStream_t st);
// det_ctd.hip: deep-level ConvTranspose input gradient k_ctd (gsum: + the producer block's BatchNorm-backward sums).  supported: as det_ctf_supported
long det_ctd_supported(int Cup, int Cout, int dtype);
int det_ctd_launch(const void* g, const void* wpk, void* dx, int Cup, int Cout, int N, int h, int w, int H, int W, hipStream_t st, const void* x,
                   const float* tr, const float* saved, double* gsum);
// det_rs32.hip: fp32 ConvTranspose weight AND bias gradient as row-streaming waves.  supported: fp32, Cup in {16, 32}, Cout in {8, 16, 32}
long det_rs32_ctw_supported(int Cup, int Cout, int dtype);
long det_rs32_ctw_ws_floats(int Cup, int Cout, int N, int h, int w, int dtype);  // 0 where not supported
int det_rs32_ctw_launch(const float* x, const float* tr, const float* g, float* dW, float* dbias, float* ws, int Cup, int Cout, int N, int h, int w, int H,
                        int W, hipStream_t st);

// det_defer.hip: the deferral window (ocrs_bwd_defer_begin .. _flush).  Scratch for one launch (null outside the window or when it is used up) and
// the queue of deferred weight-gradient reductions: columns [0, n0) of ws[nb][nelem] += into d0[(e / cin0) * ldw0 + e % cin0], columns
// [n0, n0 + n1) into d1[e - n0]
double* bwd_defer_scratch(int ndoubles);
float* bwd_defer_ws(long nfloats);  // per-block-partial workspace for launches whose entry points take none (null: not deferring / used up)
bool bwd_defer_reduce(const float* ws, int nb, int nelem, float* d0, int n0, int cin0, int ldw0, float* d1, int n1);  // false: not queued
void bwd_reduce_or_defer(const float* ws, int nb, int nelem, float* d0, int n0, int cin0, int ldw0, float* d1, int n1, hipStream_t st);  // queue, or one-job launch now

// det_rs.hip: row-streaming forms of the matrix-core block kernels, towards det_mm.hip, which owns the C entry points (ocrs_mm_bwd / ocrs_mm_fwd).
// backward supported: direct gradient, Cin / Cout in {8, 16}, and the row-streaming kernel covers the launch
bool rs_bwd_supported(int Ca, int Cb, int Cout, int pooled, int N, int H, int W);
// number of per-block partials the launch writes to ws (each PART = Cout * Cin + 11 * Cin floats, the layout k_mm_bwd_reduce sums)
int rs_bwd_blocks(int Cin, int Cout, int N, int H, int W, int g2);
int rs_bwd_launch(const Src2<bf16>& x, const float* tra, const float* trb, const float* wdw, const float* wpw, int ldw, const bf16* g1, const bf16* g2,
                  const bf16* z, const float* bn, const float* coef, bf16* gxa, bf16* gxb, float* ws, bool stats, int Cout, int N, int H, int W,
                  const BnFin& fin, hipStream_t st, const float* gl = nullptr, const float* whead = nullptr,
                  const bf16* xu = nullptr, const float* wexp = nullptr,  // gl / whead: k_rs_bwd<..., HEAD>; xu / wexp: k_rs_bwd<..., XU>
                  const BwdLast& bl = BwdLast{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0},  // bl.raw: the producers' sums finalised by the last workgroup
                  const float* img = nullptr, double* c1acc = nullptr);  // img / c1acc (with xu): k_rs_bwd<..., C1> -- the first block's sums, no dx~ store
// forward supported: Cin = 8 from one source or from the first block's u plane, or Cin = 16 from one source or the 8 | 8 concat; Cout = 8; no fused pooling
bool rs_fwd_supported(int Ca, int Cb, int Cout, int N, int H, int W);
int rs_fwd_blocks(int N, int H, int W);  // = the number of per-block statistics partials [Cout][2] the launch writes
int rs_fwd_launch(const Src2<bf16>& x, const bf16* xu, const float* wexp, const float* tra, const float* trb, const float* wdw, const float* wpw, bf16* z, float* ws,
                  int Cout, int N, int H, int W, int nb, const FwdFin& fin, hipStream_t st);
