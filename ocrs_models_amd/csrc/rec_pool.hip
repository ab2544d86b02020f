// Element-wise and reduction passes of the CRNN recogniser (gfx950): everything around its convolutions that touches a whole activation tensor.
// Reference: ocrs_models/models.py:197-242.
//
//  k_act_pool_fwd / k_rec_bn_reduce / k_dz_apply    BN + ReLU (+ MaxPool (2,2) | (2,1), floor mode) forward / backward pieces, window shape at compile time
//  k_avgpool_*     BN (no ReLU) + AvgPool2d((4,1)) on H=5, written directly as the (T, N, C) GRU input, and its backward pieces
//  k_col_sum*      per-column sums (bias gradients); rec_defer_partials makes such sums bit-reproducible inside a deferral window
#include "rec_internal.h"

// Block-level sums of the per-thread partials s1 / s2 (thread t holds the 8 channels of group t % (C / 8)) in a FIXED order -- every thread
// parks its values in LDS, thread o < 2 C then adds the 256 / CG contributions of its channel in thread order (float LDS atomics complete in
// arrival order: the statistics differed in their last bits from run to run) -- then ONE fp64 atomic per block and channel (an fp64 sum of
// fp32 partials is exact, hence order-independent; DESIGN.md "Reproducibility").
__device__ __forceinline__ void group_sums_to_gsum(const float (&s1)[8], const float (&s2)[8], int C, double* __restrict__ gsum) {
    __shared__ float s_all[256][17];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        s_all[threadIdx.x][i] = s1[i];
        s_all[threadIdx.x][8 + i] = s2[i];
    }
    __syncthreads();
    const int CG = C / 8;
    for (int o = threadIdx.x; o < 2 * C; o += 256) {
        const int which = o >= C ? 1 : 0, c = o - which * C, col = which * 8 + (c & 7);
        float a = 0.f;
        for (int t = c >> 3; t < 256; t += CG) a += s_all[t][col];
        atomicAdd(&gsum[o], (double)a);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The three window passes for the window shapes the model has -- (2,2), (2,1), (1,1): window shape known at compile time, every load of a cell
// issued before the first use (waiting for each window element in turn: 3.3-3.9 TB/s).  Floor mode: H / PH x W / PW windows, a last row / column
// that H % PH or W % PW leaves over lies in no window.  The forward and the reduction walk the windows and index z by H and W, so they take such
// tensors as they are; only k_dz_apply, which writes every pixel of dz, has a variant for them (EDGE).  The gradient goes to the FIRST maximum
// of a window.
//
// out = maxpool_{PHxPW}( max(z*scale+shift, lo) )  (BN+ReLU+MaxPool, or ReLU+MaxPool with identity scale/shift)
template <class T, int PH, int PW>
__global__ __launch_bounds__(256) void k_act_pool_fwd(const T* __restrict__ z, const float* __restrict__ tr, T* __restrict__ out, int C, int N, int H,
                                                      int W) {
    const int CG = C / 8, Hp = H / PH, Wp = W / PW;
    // the grid's thread count is a multiple of CG (256 % CG == 0): a thread keeps its channel group, whose parameters live in registers
    const long gtid = (long)blockIdx.x * 256 + threadIdx.x, nthr = (long)gridDim.x * 256;
    const int c0 = (int)(gtid % CG) * 8;
    float sc[8], sh[8], lo[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        sc[i] = tr[c0 + i];
        sh[i] = tr[C + c0 + i];
        lo[i] = tr[2 * C + c0 + i];
    }
    const long Pp = (long)N * Hp * Wp;
    for (long pp = gtid / CG; pp < Pp; pp += nthr / CG) {
        const PixIdx q = decode_pixel(pp, Hp, Wp);
        const T* zb = z + (((long)q.n * H + q.h * PH) * W + q.w * PW) * C + c0;
        Raw8<T> raw[PH * PW];
#pragma unroll
        for (int k = 0; k < PH * PW; ++k) raw[k] = load8_raw(zb + ((long)(k / PW) * W + k % PW) * C);
        float m[8];
#pragma unroll
        for (int k = 0; k < PH * PW; ++k) {
            float v[8];
            unpack8(raw[k], v);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float y = fmaxf(fmaf(v[i], sc[i], sh[i]), lo[i]);
                m[i] = k == 0 ? y : fmaxf(m[i], y);
            }
        }
        store8(out + pp * C + c0, m);
    }
}

// BN-backward reductions through ReLU (+ max-pool PHxPW): gsum[0][c] = sum ghat, gsum[1][c] = sum ghat * zhat.  g is at pooled resolution.
template <class T, int PH, int PW>
__global__ __launch_bounds__(256) void k_rec_bn_reduce(const T* __restrict__ g, const T* __restrict__ z, const float* __restrict__ bn,
                                                       const float* __restrict__ saved, double* __restrict__ gsum, int C, int N, int H, int W) {
    const int CG = C / 8, Hp = H / PH, Wp = W / PW;
    const long gtid = (long)blockIdx.x * 256 + threadIdx.x, nthr = (long)gridDim.x * 256;
    const int c0 = (int)(gtid % CG) * 8;
    float s1[8] = {0, 0, 0, 0, 0, 0, 0, 0}, s2[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    float sc[8], sh[8], mu[8], rs[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        sc[i] = bn[c0 + i];
        sh[i] = bn[C + c0 + i];
        mu[i] = saved[c0 + i];
        rs[i] = saved[C + c0 + i];
    }
    const long Pp = (long)N * Hp * Wp;
    for (long pp = gtid / CG; pp < Pp; pp += nthr / CG) {
        const PixIdx q = decode_pixel(pp, Hp, Wp);
        const T* zb = z + (((long)q.n * H + q.h * PH) * W + q.w * PW) * C + c0;
        const Raw8<T> graw = load8_raw(g + pp * C + c0);
        Raw8<T> raw[PH * PW];
#pragma unroll
        for (int k = 0; k < PH * PW; ++k) raw[k] = load8_raw(zb + ((long)(k / PW) * W + k % PW) * C);
        float gv[8], best[8], bz[8];
        unpack8(graw, gv);
#pragma unroll
        for (int k = 0; k < PH * PW; ++k) {
            float zv[8];
            unpack8(raw[k], zv);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float y = fmaxf(fmaf(zv[i], sc[i], sh[i]), 0.f);
                if (k == 0 || y > best[i]) {
                    best[i] = y;
                    bz[i] = zv[i];
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float gh = best[i] > 0.f ? gv[i] : 0.f;
            s1[i] += gh;
            s2[i] = fmaf(gh, (bz[i] - mu[i]) * rs[i], s2[i]);
        }
    }
    group_sums_to_gsum(s1, s2, C, gsum);
}

// NTB threads per block: 256, or 1024 when the column sums are asked for (a quarter of the trailing same-address atomics at the same occupancy:
// with 256-thread blocks the atomic tail made the fused pass slower than dz_apply + a separate column-sum kernel)
//
// dz = coefA * ghat + coefB * z + coefC for every pixel (ghat routed through ReLU and the PHxPW max-pool).  With bn = identity and coef = (1,0,0)
// this is the plain ReLU(+pool) backward.  EDGE = false: the windows tile the tensor exactly.  EDGE = true (H % PH or W % PW left over): the same
// pass over the grid of cells including the partial last row / column; pixels in no full window get coefB*z + coefC.
template <class T, int PH, int PW, bool EDGE, int NTB>
__global__ __launch_bounds__(NTB) void k_dz_apply(const T* __restrict__ g, const T* __restrict__ z, const float* __restrict__ bn,
                                                  const float* __restrict__ coef, T* __restrict__ dz, int C, int N, int H, int W,
                                                  float* __restrict__ dsum /*nullable [C]: += column sums of the stored dz (a bias gradient)*/,
                                                  float* __restrict__ dsum_ws /*nullable: per-block partials [gridDim.x][C] instead of the atomics (rec_defer_partials)*/) {
    const int CG = C / 8, Hp = H / PH, Wp = W / PW;
    const int Hc = EDGE ? (H + PH - 1) / PH : Hp, Wc = EDGE ? (W + PW - 1) / PW : Wp;  // the cell grid
    const long gtid = (long)blockIdx.x * NTB + threadIdx.x, nthr = (long)gridDim.x * NTB;
    const int c0 = (int)(gtid % CG) * 8;  // (fixed per thread, see k_act_pool_fwd)
    float sc[8], sh[8], ca[8], cb[8], cc[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        sc[i] = bn[c0 + i];
        sh[i] = bn[C + c0 + i];
        ca[i] = coef[c0 + i];
        cb[i] = coef[C + c0 + i];
        cc[i] = coef[2 * C + c0 + i];
    }
    float ds[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const long Pp = (long)N * Hc * Wc;
    for (long pp = gtid / CG; pp < Pp; pp += nthr / CG) {
        const PixIdx q = decode_pixel(pp, Hc, Wc);
        const long zoff = (((long)q.n * H + q.h * PH) * W + q.w * PW) * C + c0;  // (the cell's first pixel always lies inside the tensor)
        // EDGE: a partial cell has no gradient (its load is pointed at z and not used) and its pixels outside the tensor re-read the first one (not stored)
        const bool full = !EDGE || (q.h < Hp && q.w < Wp);
        auto inside = [&](int k) { return q.h * PH + k / PW < H && q.w * PW + k % PW < W; };  // (asked under EDGE only)
        const Raw8<T> graw = load8_raw(!EDGE ? g + pp * C + c0 : (full ? g + (((long)q.n * Hp + q.h) * Wp + q.w) * C + c0 : z + zoff));
        Raw8<T> raw[PH * PW];
#pragma unroll
        for (int k = 0; k < PH * PW; ++k) raw[k] = load8_raw(z + zoff + ((!EDGE || inside(k)) ? ((long)(k / PW) * W + k % PW) * C : 0));
        float gv[8], zs[PH * PW][8], best[8];
        int bk[8];
        unpack8(graw, gv);
#pragma unroll
        for (int k = 0; k < PH * PW; ++k) {
            unpack8(raw[k], zs[k]);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float y = fmaxf(fmaf(zs[k][i], sc[i], sh[i]), 0.f);
                if (k == 0 || y > best[i]) {
                    best[i] = y;
                    bk[i] = k;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < PH * PW; ++k) {
            if (EDGE && !inside(k)) continue;
            float o[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float gh = (full && bk[i] == k && best[i] > 0.f) ? gv[i] : 0.f;
                o[i] = fmaf(ca[i], gh, fmaf(cb[i], zs[k][i], cc[i]));
                if (dsum) ds[i] += Elem<T>::round(o[i]);
            }
            store8(dz + zoff + ((long)(k / PW) * W + k % PW) * C, o);
        }
    }
    if (dsum) {  // (kernel-uniform) fixed-order block sums, then one fp32 atomic per block and channel, like k_col_sum4's
        __shared__ float s_all[NTB][9];
#pragma unroll
        for (int i = 0; i < 8; ++i) s_all[threadIdx.x][i] = ds[i];
        __syncthreads();
        for (int c = threadIdx.x; c < C; c += NTB) {
            float a = 0.f;
            for (int t = c >> 3; t < NTB; t += CG) a += s_all[t][c & 7];
            if (dsum_ws) dsum_ws[(long)blockIdx.x * C + c] = a;
            else atomicAdd(&dsum[c], a);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// BatchNorm2d (no ReLU) + AvgPool2d((4,1)) on H=5 (models.py:234-242) written as the GRU input seq[t=w][n][c] (fp32):
//   seq = mean_{h<4}(z[n][h][w][c]) * scale + shift
template <class T>
__global__ __launch_bounds__(256) void k_avgpool_fwd(const T* __restrict__ z, const float* __restrict__ tr, float* __restrict__ seq, int C, int N, int H,
                                                     int W) {
    const int CG = C / 8;
    const long total = (long)N * W * CG;
    for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < total; it += (long)gridDim.x * 256) {
        const long nw = it / CG;
        const int c0 = (int)(it - nw * CG) * 8;
        const int n = (int)(nw / W), w = (int)(nw - (long)n * W);
        float s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int h = 0; h < 4; ++h) {
            float v[8];
            load8(z + (((long)n * H + h) * W + w) * C + c0, v);
#pragma unroll
            for (int i = 0; i < 8; ++i) s[i] += v[i];
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) s[i] = fmaf(s[i] * 0.25f, tr[c0 + i], tr[C + c0 + i]);
        store8(seq + ((long)w * N + n) * C + c0, s);
    }
}

// reductions for its backward: ghat[n][h<4][w][c] = gseq[w][n][c] / 4, row 4: 0.  BN count = N*H*W.
template <class T>
__global__ __launch_bounds__(256) void k_avgpool_bn_reduce(const float* __restrict__ gseq, const T* __restrict__ z, const float* __restrict__ saved,
                                                           double* __restrict__ gsum, int C, int N, int H, int W) {
    const int CG = C / 8;
    const long gtid = (long)blockIdx.x * 256 + threadIdx.x, nthr = (long)gridDim.x * 256;
    const int c0 = (int)(gtid % CG) * 8;
    float s1[8] = {0, 0, 0, 0, 0, 0, 0, 0}, s2[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    float mu[8], rs[8];  // (per-thread channel group: parameters in registers, all five loads of a column issued before the first use)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        mu[i] = saved[c0 + i];
        rs[i] = saved[C + c0 + i];
    }
    for (long nw = gtid / CG; nw < (long)N * W; nw += nthr / CG) {
        const int n = (int)(nw / W), w = (int)(nw - (long)n * W);
        float gv[8];
        Raw8<T> raw[4];
#pragma unroll
        for (int h = 0; h < 4; ++h) raw[h] = load8_raw(z + (((long)n * H + h) * W + w) * C + c0);
        load8(gseq + ((long)w * N + n) * C + c0, gv);
        float zs[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            float v[8];
            unpack8(raw[h], v);
#pragma unroll
            for (int i = 0; i < 8; ++i) zs[i] += (v[i] - mu[i]) * rs[i];
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            s1[i] += gv[i];
            s2[i] = fmaf(gv[i] * 0.25f, zs[i], s2[i]);
        }
    }
    group_sums_to_gsum(s1, s2, C, gsum);
}

template <class T>
__global__ __launch_bounds__(256) void k_avgpool_dz(const float* __restrict__ gseq, const T* __restrict__ z, const float* __restrict__ coef,
                                                    T* __restrict__ dz, int C, int N, int H, int W) {
    const int CG = C / 8;
    const long total = (long)N * H * W * CG;
    for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < total; it += (long)gridDim.x * 256) {
        const long p = it / CG;
        const int c0 = (int)(it - p * CG) * 8;
        const PixIdx q = decode_pixel(p, H, W);
        float zv[8], gv[8] = {0, 0, 0, 0, 0, 0, 0, 0}, o[8];
        load8(z + p * C + c0, zv);
        if (q.h < 4) load8(gseq + ((long)q.w * N + q.n) * C + c0, gv);
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = fmaf(coef[c0 + i], gv[i] * 0.25f, fmaf(coef[C + c0 + i], zv[i], coef[2 * C + c0 + i]));
        store8(dz + p * C + c0, o);
    }
}

// per-column sum of a [rows][ld] fp32/bf16 matrix (bias gradients)
// ws (nullable, round 5): per-block partials [gridDim.x][C] instead of the cross-block float atomics -- summed in a fixed order by the deferred
// reduce launch (ocrs_bwd_defer_begin / _flush, det_defer.hip).  The in-block sums are fixed-order slots (no LDS float atomics) either way.
template <class T>
__global__ __launch_bounds__(256) void k_col_sum(const T* __restrict__ a, int ld, int C, float* __restrict__ out, long rows, float* __restrict__ ws) {
    extern __shared__ float s_acc[];  // [2 row phases][C]
    const int c = threadIdx.x % 128;
    const int sub = threadIdx.x / 128;
    for (int cb = 0; cb < C; cb += 128) {
        if (cb + c < C) {
            float s = 0.f;
            for (long r = (long)blockIdx.x * 2 + sub; r < rows; r += (long)gridDim.x * 2) s += Elem<T>::ld(a + r * ld + cb + c);
            s_acc[sub * C + cb + c] = s;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < C; i += 256) {
        const float v = s_acc[i] + s_acc[C + i];
        if (ws) ws[(long)blockIdx.x * C + i] = v;
        else atomicAdd(&out[i], v);
    }
}

// The same for C % 4 == 0 and 4-element-aligned rows: a thread owns 4 consecutive columns (one 16 / 8-byte load per row), 64 column quads
// x 4 row phases per block, four rows in flight per thread; per-block partials pre-reduced in LDS, then C atomics per block (grid <= 2/CU).
template <class T>
__global__ __launch_bounds__(256) void k_col_sum4(const T* __restrict__ a, int ld, int C, float* __restrict__ out, long rows, float* __restrict__ ws) {
    extern __shared__ float s_acc[];  // [4 row phases][C]
    const int cq = threadIdx.x & 63, ph = threadIdx.x >> 6;
    const long rstep = (long)gridDim.x * 4;
    for (int cb = 0; cb < C; cb += 256) {
        const int c = cb + cq * 4;
        if (c < C) {
            float s[4] = {0.f, 0.f, 0.f, 0.f};
            long r = (long)blockIdx.x * 4 + ph;
            for (; r + 7 * rstep < rows; r += 8 * rstep) {  // eight rows in flight per thread (2 blocks per CU: 64 KB in flight per CU)
                float v[8][4];
#pragma unroll
                for (int u = 0; u < 8; ++u) load4(a + (r + u * rstep) * ld + c, v[u]);
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    s[i] += ((v[0][i] + v[1][i]) + (v[2][i] + v[3][i])) + ((v[4][i] + v[5][i]) + (v[6][i] + v[7][i]));
            }
            for (; r + 3 * rstep < rows; r += 4 * rstep) {
                float v[4][4];
#pragma unroll
                for (int u = 0; u < 4; ++u) load4(a + (r + u * rstep) * ld + c, v[u]);
#pragma unroll
                for (int i = 0; i < 4; ++i) s[i] += (v[0][i] + v[1][i]) + (v[2][i] + v[3][i]);
            }
            for (; r < rows; r += rstep) {
                float v[4];
                load4(a + r * ld + c, v);
#pragma unroll
                for (int i = 0; i < 4; ++i) s[i] += v[i];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) s_acc[ph * C + c + i] = s[i];
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < C; i += 256) {
        const float v = (s_acc[i] + s_acc[C + i]) + (s_acc[2 * C + i] + s_acc[3 * C + i]);
        if (ws) ws[(long)blockIdx.x * C + i] = v;
        else atomicAdd(&out[i], v);
    }
}

// Deferred mode (ocrs_bwd_defer_begin .. _flush): a launch that would end in cross-block float atomics onto out [n] writes per-block partials
// [nb][n] instead and queues their fixed-order column sum (k_reduce_multi, det_defer.hip) -- the sums become bit-reproducible.  Returns the partial
// buffer, or null (not deferring / pool or queue full): the launch then falls back to the atomics.
float* rec_defer_partials(int nb, int n, float* out) {
    float* ws = bwd_defer_ws((long)nb * n);
    if (!ws) return nullptr;
    if (!bwd_defer_reduce(ws, nb, n, out, n, n, n, nullptr, 0)) return nullptr;
    return ws;
}

// ---------------------------------------------------------------------------------------------------------------------
// What the window kernels are built for: the model's windows (2,2), (2,1), (1,1), and C / 8 channel groups that divide the 256 threads of a block
// (a thread keeps its group).  with_window calls f(T{}, Win<PH, PW, EDGE>{}) with the element type, the window and -- k_dz_apply's concern -- whether
// the windows leave a last row or column over, as compile-time constants.
template <int PH_, int PW_, bool EDGE_>
struct Win {
    static constexpr int PH = PH_, PW = PW_;
    static constexpr bool EDGE = EDGE_;
};
static bool window_ok(int C, int PH, int PW) {
    return C >= 8 && C % 8 == 0 && 256 % (C / 8) == 0 && ((PH == 2 && (PW == 2 || PW == 1)) || (PH == 1 && PW == 1));
}
template <class F>
static void with_window(int dtype, int PH, int PW, bool edge, F&& f) {
    with_dtype(dtype, [&](auto t) {
        if (PH == 1) f(t, Win<1, 1, false>{});
        else if (PW == 1) edge ? f(t, Win<2, 1, true>{}) : f(t, Win<2, 1, false>{});
        else edge ? f(t, Win<2, 2, true>{}) : f(t, Win<2, 2, false>{});
    });
}

extern "C" {

// BN+ReLU(+MaxPool PHxPW) forward on a pre-BN tensor z (models.py:197-199, 214-216, 231-233); tr = [3][C] load transform.
// All three window entry points: windows (2,2), (2,1), (1,1) in floor mode (a last row / column that H % PH or W % PW leaves over is in no window),
// C / 8 a power of two <= 256; anything else is OCRS_ERR_ARG.
int ocrs_act_pool_fwd(const void* z, const float* tr, void* out, int C, int N, int H, int W, int PH, int PW, int dtype, hipStream_t st) {
    OCRS_CHECK_ARG(z && tr && out && window_ok(C, PH, PW));
    const int grid = ew_grid((long)N * (H / PH) * (W / PW) * (C / 8));
    with_window(dtype, PH, PW, false, [&](auto t, auto w) {
        using T = decltype(t);
        using Wn = decltype(w);
        hipLaunchKernelGGL((k_act_pool_fwd<T, Wn::PH, Wn::PW>), dim3(grid), dim3(256), 0, st, (const T*)z, tr, (T*)out, C, N, H, W);
    });
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}
// backward reductions (gsum [2][C] double, ACCUMULATED: the caller zeroes it) and dz materialisation
int ocrs_rec_bn_reduce(const void* g, const void* z, const float* bn, const float* saved, double* gsum, int C, int N, int H, int W, int PH, int PW,
                       int dtype, hipStream_t st) {
    OCRS_CHECK_ARG(g && z && bn && saved && gsum && window_ok(C, PH, PW));
    int grid = ew_grid((long)N * (H / PH) * (W / PW) * (C / 8));
    constexpr int bpc = 4;  // every block ends in 2 C same-address fp64 atomics (~11 ns each, serial per address)
    if (grid > bpc * kNumCU) grid = bpc * kNumCU;
    with_window(dtype, PH, PW, false, [&](auto t, auto w) {
        using T = decltype(t);
        using Wn = decltype(w);
        hipLaunchKernelGGL((k_rec_bn_reduce<T, Wn::PH, Wn::PW>), dim3(grid), dim3(256), 0, st, (const T*)g, (const T*)z, bn, saved, gsum, C, N, H, W);
    });
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}
int ocrs_dz_apply(const void* g, const void* z, const float* bn, const float* coef, void* dz, int C, int N, int H, int W, int PH, int PW, int dtype,
                  float* dsum, hipStream_t st) {
    OCRS_CHECK_ARG(g && z && bn && coef && dz && window_ok(C, PH, PW));
    const bool edge = H % PH != 0 || W % PW != 0;
    int grid = ew_grid((long)N * ((H + PH - 1) / PH) * ((W + PW - 1) / PW) * (C / 8));
    // the column sums ride along in the same pass (1024-thread blocks, every one ending in C same-address atomics or, deferring, a row of
    // partials), except on a tensor with a left-over row / column: there a separate pass over dz sums them
    const bool fused = dsum && !edge;
    float* dsum_ws = nullptr;
    if (fused) {
        grid = (grid + 3) / 4;
        if (grid > kNumCU) grid = kNumCU;  // one block per CU
        dsum_ws = rec_defer_partials(grid, C, dsum);
    }
    with_window(dtype, PH, PW, edge, [&](auto t, auto w) {
        using T = decltype(t);
        using Wn = decltype(w);
        if constexpr (!Wn::EDGE) {
            if (fused) {
                hipLaunchKernelGGL((k_dz_apply<T, Wn::PH, Wn::PW, false, 1024>), dim3(grid), dim3(1024), 0, st, (const T*)g, (const T*)z, bn, coef, (T*)dz,
                                   C, N, H, W, dsum, dsum_ws);
                return;
            }
        }
        hipLaunchKernelGGL((k_dz_apply<T, Wn::PH, Wn::PW, Wn::EDGE, 256>), dim3(grid), dim3(256), 0, st, (const T*)g, (const T*)z, bn, coef, (T*)dz, C, N,
                           H, W, (float*)nullptr, (float*)nullptr);
    });
    OCRS_LAUNCH_CHECK();
    if (dsum && !fused) return ocrs_col_sum(dz, C, C, dsum, (long)N * H * W, dtype, st);
    return OCRS_OK;
}

// BatchNorm2d + AvgPool2d((4,1)) on H=5 + permute to (T=W, N, C) fp32 (models.py:241-242, 259-262), and its backward pieces.
// All three compute ONE pooled row from rows 0..3 (rows 4.. lie in no window): that is AvgPool2d((4,1)) for 4 <= H <= 7 only; any other H is
// OCRS_ERR_ARG (H < 4 would read past the image, H >= 8 has a second pooled row).
static bool avgpool_ok(int C, int H) { return C >= 8 && C % 8 == 0 && H >= 4 && H <= 7; }
int ocrs_avgpool_fwd(const void* z, const float* tr, float* seq, int C, int N, int H, int W, int dtype, hipStream_t st) {
    OCRS_CHECK_ARG(z && tr && seq && avgpool_ok(C, H));
    const int grid = ew_grid((long)N * W * (C / 8));
    if (dtype == 1)
        hipLaunchKernelGGL(k_avgpool_fwd<bf16>, dim3(grid), dim3(256), 0, st, (const bf16*)z, tr, seq, C, N, H, W);
    else
        hipLaunchKernelGGL(k_avgpool_fwd<float>, dim3(grid), dim3(256), 0, st, (const float*)z, tr, seq, C, N, H, W);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}
int ocrs_avgpool_bn_reduce(const float* gseq, const void* z, const float* saved, double* gsum, int C, int N, int H, int W, int dtype, hipStream_t st) {
    OCRS_CHECK_ARG(gseq && z && saved && gsum && avgpool_ok(C, H) && 256 % (C / 8) == 0);
    int grid = ew_grid((long)N * W * (C / 8));
    if (grid > 4 * kNumCU) grid = 4 * kNumCU;  // (ends in 2 C same-address fp64 atomics per block: see ocrs_rec_bn_reduce)
    if (dtype == 1)
        hipLaunchKernelGGL(k_avgpool_bn_reduce<bf16>, dim3(grid), dim3(256), 2 * C * sizeof(float), st, gseq, (const bf16*)z, saved, gsum, C, N, H, W);
    else
        hipLaunchKernelGGL(k_avgpool_bn_reduce<float>, dim3(grid), dim3(256), 2 * C * sizeof(float), st, gseq, (const float*)z, saved, gsum, C, N, H, W);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}
int ocrs_avgpool_dz(const float* gseq, const void* z, const float* coef, void* dz, int C, int N, int H, int W, int dtype, hipStream_t st) {
    OCRS_CHECK_ARG(gseq && z && coef && dz && avgpool_ok(C, H));
    const int grid = ew_grid((long)N * H * W * (C / 8));
    if (dtype == 1)
        hipLaunchKernelGGL(k_avgpool_dz<bf16>, dim3(grid), dim3(256), 0, st, gseq, (const bf16*)z, coef, (bf16*)dz, C, N, H, W);
    else
        hipLaunchKernelGGL(k_avgpool_dz<float>, dim3(grid), dim3(256), 0, st, gseq, (const float*)z, coef, (float*)dz, C, N, H, W);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

// column sums (bias gradients): out[c] += sum_rows a[row][c]
int ocrs_col_sum(const void* a, int ld, int C, float* out, long rows, int dtype, hipStream_t st) {
    OCRS_CHECK_ARG(a && out && C > 0 && ld >= C && rows > 0);
    const int esz = dtype == 1 ? 2 : 4;
    if (C % 4 == 0 && ld % 4 == 0 && (reinterpret_cast<uintptr_t>(a) & (4 * esz - 1)) == 0) {
        long g4 = (rows + 15) / 16;  // >= 4 rows per thread before another block is worth its C trailing atomics
        if (g4 > 2 * kNumCU) g4 = 2 * kNumCU;
        if (g4 < 1) g4 = 1;
        float* ws = rec_defer_partials((int)g4, C, out);  // (deferring: per-block partials + one queued fixed-order reduce instead of float atomics)
        if (dtype == 1)
            hipLaunchKernelGGL(k_col_sum4<bf16>, dim3((int)g4), dim3(256), 4 * C * sizeof(float), st, (const bf16*)a, ld, C, out, rows, ws);
        else
            hipLaunchKernelGGL(k_col_sum4<float>, dim3((int)g4), dim3(256), 4 * C * sizeof(float), st, (const float*)a, ld, C, out, rows, ws);
        OCRS_LAUNCH_CHECK();
        return OCRS_OK;
    }
    long g = (rows + 1) / 2;
    if (g > 1024) g = 1024;
    float* ws = rec_defer_partials((int)g, C, out);
    if (dtype == 1)
        hipLaunchKernelGGL(k_col_sum<bf16>, dim3((int)g), dim3(256), 2 * C * sizeof(float), st, (const bf16*)a, ld, C, out, rows, ws);
    else
        hipLaunchKernelGGL(k_col_sum<float>, dim3((int)g), dim3(256), 2 * C * sizeof(float), st, (const float*)a, ld, C, out, rows, ws);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

}  // extern "C"
