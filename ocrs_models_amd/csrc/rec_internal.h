// Host-side internals the recogniser's files share (C++ linkage; the C ABI is include/ocrs_hip.h).  Included by the file that defines each
// function and by every file that calls it.
#pragma once
#include "det_internal.h"  // the deferral queue (bwd_defer_*, det_defer.hip)

// rec_pool.hip: partial buffer [nb][n] + queued fixed-order column sum into out [n] (null: not deferring -- the launch keeps its atomics)
float* rec_defer_partials(int nb, int n, float* out);

// The specialised 3x3 forward kernels ocrs_conv_igemm (rec_conv.hip) tries before the generic k_conv_igemm: *_supported tells whether the kernel
// takes the call, *_launch runs it.
// rec_conv4.hip: narrow layers, weights resident in LDS
bool conv3x3_tile_supported(int ldx, int ldo, int Cin, int M, int Hi, int Wi, int Ho, int Wo, int KH, int KW, int padh, int padw, int dtype);
int conv3x3_tile_launch(const void* x, int ldx, const void* wpk, void* out, int ldo, const float* bias, int relu, double* gstat, int Cin, int M, int N, int H, int W,
                        hipStream_t st);
// rec_conv3.hip: whole-row passes, one workgroup per CU
bool conv3x3_rows_supported(int ldx, int ldo, int Cin, int M, int Hi, int Wi, int Ho, int Wo, int KH, int KW, int padh, int padw, int dtype);
int conv3x3_rows_launch(const void* x, int ldx, const void* wpk, void* out, int ldo, const float* bias, int relu, double* gstat, int Cin, int M, int N, int Hi, int Wi,
                        int Ho, int Wo, int KW, int pad, hipStream_t st);
// rec_conv2.hip: the 128-output-channel layers, 128 x 256 block tiles
bool conv3x3_c128_supported(int ldx, int ldo, int Cin, int M, int Hi, int Wi, int Ho, int Wo, int KH, int KW, int padh, int padw, int dtype);
int conv3x3_c128_launch(const void* x, int ldx, const void* wpk, void* out, int ldo, const float* bias, int relu, double* gstat, int Cin, int N, int H, int W,
                        hipStream_t st);
