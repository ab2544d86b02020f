// The generic implicit-GEMM convolution of the CRNN recogniser (gfx950).  Reference: ocrs_models/models.py:179-251.
//
//  k_conv_igemm    implicit-GEMM KHxKW convolution on MFMA (also plain GEMM with KH=KW=1): forward, dgrad (flipped weights),
//                  GRU input projections, Linear.  Input tile (+halo) of 32 channels staged once in LDS; the nine taps read
//                  MFMA B-fragments straight from that tile at shifted pixel offsets (no im2col buffer).
//  ocrs_conv_igemm tries the specialised 3x3 kernels first (rec_conv2.hip, rec_conv3.hip, rec_conv4.hip) and runs k_conv_igemm for the rest.
// The recogniser's other kernels: rec_conv0.hip (first layer), rec_wgrad.hip (weight gradients), rec_pool.hip (BN + ReLU + pooling passes,
// column sums), rec_gemm.hip (split-bf16 GEMMs of the GRU projections).
#include "rec_internal.h"

// ---------------------------------------------------------------------------------------------------------------------
// WM = waves along M: the four waves tile the block's output WM x (4 / WM) -- WM = 1: every wave computes all MT tiles for a quarter of the
// pixels; 2: half of the M tiles x half of the pixel tiles; 4: a quarter of the M tiles x all pixel tiles.  Each weight fragment is fetched
// by 4 / WM waves (the fragments come from L2 -- 72 KB per 32-channel chunk for MT = 8 -- and their re-fetch by every wave was the kernel's
// largest data stream), each pixel fragment is read from LDS by WM waves.
template <class T, int MT, int TH, int TW, int WM = 1>
__global__ __launch_bounds__(256) void k_conv_igemm(const T* __restrict__ x, int ldx, const void* __restrict__ wpk, T* __restrict__ out, int ldo,
                                                    const float* __restrict__ bias, int relu, double* __restrict__ gstat, int Cin, int M,
                                                    int MT_total, int N, int Hi, int Wi, int Ho, int Wo, int KH, int KW, int padh, int padw) {
    constexpr int PITCH = RecTile<T>::PITCH;
    constexpr int NTILES = TH * TW / 16, PTW = NTILES * WM / 4, TPR = TW / 16;  // N-tiles per block / per wave / per tile row
    constexpr int MTW = MT / WM;                                                // M-tiles per wave
    static_assert(NTILES % 4 == 0 && TW % 16 == 0 && MT % WM == 0 && (WM == 1 || WM == 2 || WM == 4), "tile shape");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* xs = reinterpret_cast<T*>(smem);  // [(TH+KH-1)*(TW+KW-1)][PITCH]
    const int HWp = TW + KW - 1, HHp = TH + KH - 1, HP = HWp * HHp;
    float* s_stat = reinterpret_cast<float*>(smem + ((HP * PITCH * sizeof(T) + 15) & ~15));  // [4 / WM][2][MT*16]: one slot per pixel-wave
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mt0 = blockIdx.y * MT;
    const int mw0 = (wave % WM) * MTW;  // first M tile (within the block's MT) of this wave
    if (gstat) {
        for (int i = tid; i < (4 / WM) * 2 * MT * 16; i += 256) s_stat[i] = 0.f;
        __syncthreads();
    }
    const int tiles_x = (Wo + TW - 1) / TW, tiles_y = (Ho + TH - 1) / TH;
    const int ntiles = N * tiles_x * tiles_y;
    const int ncc = Cin / 32;
    int oty[PTW], otx[PTW];
#pragma unroll
    for (int a = 0; a < PTW; ++a) {
        const int q = (wave / WM) * PTW + a;
        oty[a] = q / TPR;
        otx[a] = (q % TPR) * 16;
    }
    TileSched ts(ntiles);
    for (long t = ts.first; t < ts.end; t += ts.step) {
        const int tpi = tiles_x * tiles_y;
        const int n = (int)t / tpi, r = (int)t - n * tpi;
        const int h0 = (r / tiles_x) * TH, w0 = (r % tiles_x) * TW;
        f32x4 acc[PTW][MTW];
#pragma unroll
        for (int a = 0; a < PTW; ++a)
#pragma unroll
            for (int b = 0; b < MTW; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int cc = 0; cc < ncc; ++cc) {
            __syncthreads();  // previous chunk's fragment reads done
            for (int it = tid; it < HP * 4; it += 256) {
                const int hp = it >> 2, g8 = it & 3;
                const int hy = hp / HWp, hx = hp - hy * HWp;
                const int h = h0 + hy - padh, w = w0 + hx - padw;
                float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                if (h >= 0 && h < Hi && w >= 0 && w < Wi) load8(x + (((long)n * Hi + h) * Wi + w) * ldx + cc * 32 + g8 * 8, v);
                store8(xs + hp * PITCH + g8 * 8, v);
            }
            __syncthreads();
            for (int tap = 0; tap < KH * KW; ++tap) {
                const int ky = tap / KW, kx = tap - ky * KW;
                typename Mma<T>::Frag pf[PTW];
#pragma unroll
                for (int a = 0; a < PTW; ++a) pf[a] = Mma<T>::load_p(xs, PITCH, (oty[a] + ky) * HWp + otx[a] + kx, lane, 32);
                const long kc = (long)tap * ncc + cc;
#pragma unroll
                for (int b = 0; b < MTW; ++b) {
                    // M tiles past the packed weight (M = 97 -> 7 tiles, this block covers 8): read tile 0 instead and use a zero fragment.  The
                    // unguarded read ran 2 KB past the end of the packed buffer in the last K chunk -- a memory access fault whenever that
                    // buffer was the last thing in its allocator segment -- and put the next chunk's weights into the pad columns before
                    const int mtile = mt0 + mw0 + b;
                    typename Mma<T>::Frag wf = Mma<T>::load_w(wpk, kc * MT_total + (mtile < MT_total ? mtile : 0), lane);
                    if (mtile >= MT_total) wf = typename Mma<T>::Frag{};
#pragma unroll
                    for (int a = 0; a < PTW; ++a) acc[a][b] = Mma<T>::template mma<8>(wf, pf[a], acc[a][b]);
                }
            }
        }
        // epilogue
#pragma unroll
        for (int b = 0; b < MTW; ++b) {
            const int m0 = (mt0 + mw0 + b) * 16 + (lane >> 4) * 4;
            float bs[4] = {0.f, 0.f, 0.f, 0.f};
            if (bias) {
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) bs[r4] = m0 + r4 < M ? bias[m0 + r4] : 0.f;
            }
            float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int a = 0; a < PTW; ++a) {
                const int h = h0 + oty[a], w = w0 + otx[a] + (lane & 15);
                if (h < Ho && w < Wo && m0 < ldo) {
                    float v[4];
#pragma unroll
                    for (int r4 = 0; r4 < 4; ++r4) {
                        v[r4] = acc[a][b][r4] + bs[r4];
                        if (relu) v[r4] = fmaxf(v[r4], 0.f);
                    }
                    store4(out + (((long)n * Ho + h) * Wo + w) * ldo + m0, v[0], v[1], v[2], v[3]);
#pragma unroll
                    for (int r4 = 0; r4 < 4; ++r4) {
                        const float q = Elem<T>::round(v[r4]);
                        s1[r4] += q;
                        s2[r4] = fmaf(q, q, s2[r4]);
                    }
                }
            }
            if (gstat) {
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) {
                    const float a1 = quad16_sum(s1[r4]), a2 = quad16_sum(s2[r4]);
                    if ((lane & 15) == 0) {  // (wave, channel) has exactly one owner lane: plain adds in program order -> run-to-run bit-stable
                        float* slot = s_stat + (wave / WM) * 2 * MT * 16 + (mw0 + b) * 16 + (lane >> 4) * 4 + r4;
                        slot[0] += a1;
                        slot[MT * 16] += a2;
                    }
                }
            }
        }
    }
    if (gstat) {
        __syncthreads();
        for (int i = tid; i < MT * 16; i += 256) {
            const int m = mt0 * 16 + i;
            if (m < M) {
                float a1 = 0.f, a2 = 0.f;
#pragma unroll
                for (int wn = 0; wn < 4 / WM; ++wn) {
                    a1 += s_stat[wn * 2 * MT * 16 + i];
                    a2 += s_stat[wn * 2 * MT * 16 + MT * 16 + i];
                }
                atomicAdd(&gstat[m], (double)a1);  // fp64 sums of fp32 partials are exact, hence order-independent (DESIGN.md "Reproducibility")
                atomicAdd(&gstat[M + m], (double)a2);
            }
        }
    }
}

template <class T, int TH, int TW>
static int launch_igemm(const void* x, int ldx, const void* wpk, void* out, int ldo, const float* bias, int relu, double* gstat, int Cin, int M,
                        int N, int Hi, int Wi, int Ho, int Wo, int KH, int KW, int padh, int padw, hipStream_t st) {
    const int MT_total = (M + 15) / 16;
    const int tiles = N * ((Wo + TW - 1) / TW) * ((Ho + TH - 1) / TH);
    const int HP = (TH + KH - 1) * (TW + KW - 1);
#define IG(MT_)                                                                                                                                  \
    {                                                                                                                                            \
        const size_t smem = ((HP * RecTile<T>::PITCH * sizeof(T) + 15) & ~15) + 4 * 2 * MT_ * 16 * sizeof(float);                                   \
        const int gy = (MT_total + MT_ - 1) / MT_;                                                                                               \
        constexpr int WM_ = (Elem<T>::is_bf16 && TH > 1) ? (MT_ >= 8 ? 4 : (MT_ >= 4 ? 2 : 1)) : 1; /* measured: 1382 -> 974 us, 270 -> 230 us */ \
        hipLaunchKernelGGL((k_conv_igemm<T, MT_, TH, TW, WM_>), dim3(persistent_grid(tiles, gy >= 4 ? 2 : 4), gy), dim3(256), smem, st, (const T*)x, ldx, \
                           wpk, (T*)out, ldo, bias, relu, gstat, Cin, M, MT_total, N, Hi, Wi, Ho, Wo, KH, KW, padh, padw);                         \
    }
    if (MT_total % 8 == 0 || MT_total > 8)
        IG(8)
    else if (MT_total % 4 == 0 || MT_total > 4)
        IG(4)
    else if (MT_total >= 2)
        IG(2)
    else
        IG(1)
#undef IG
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

extern "C" {

// The kernel ocrs_conv_igemm runs for these arguments (its dispatch below, restated for callers that must know what they exercised):
// 1 = k_conv3x3_tile (rec_conv4.hip), 2 = k_conv3x3_rows (rec_conv3.hip), 3 = k_conv3x3_c128 (rec_conv2.hip), 0 = the generic k_conv_igemm.
long ocrs_conv_igemm_kernel(int ldx, int ldo, int Cin, int M, int Hi, int Wi, int Ho, int Wo, int KH, int KW, int padh, int padw, int dtype) {
    if (conv3x3_tile_supported(ldx, ldo, Cin, M, Hi, Wi, Ho, Wo, KH, KW, padh, padw, dtype)) return 1;
    if (conv3x3_rows_supported(ldx, ldo, Cin, M, Hi, Wi, Ho, Wo, KH, KW, padh, padw, dtype)) return 2;
    if (conv3x3_c128_supported(ldx, ldo, Cin, M, Hi, Wi, Ho, Wo, KH, KW, padh, padw, dtype)) return 3;
    return 0;
}

// Implicit-GEMM convolution / GEMM:  out[n][ho][wo][m] = sum_{ky,kx,c} W[m][(ky,kx,c)] * x[n][ho+ky-padh][wo+kx-padw][c]  (+bias, ReLU)
//   nn.Conv2d forward (models.py:189-240), its dgrad (flipped packed weights), GRU input projections and nn.Linear (KH=KW=1, Hi=Ho=1).
//   x [N][Hi][Wi][ldx] (Cin % 32 == 0, ldx >= Cin); wpk = ocrs_pack_frags(K = KH*KW*Cin ordered (tap, c), M); out [N][Ho][Wo][ldo];
//   gstat (nullable): [2][M] double batch sums of the (rounded) outputs, ACCUMULATED: the caller zeroes it (one fill for all layers of a step, like ocrs_dwpw_fwd).  Outputs rows m in [M, ldo) are written as 0(+0 bias).
int ocrs_conv_igemm(const void* x, int ldx, const void* wpk, void* out, int ldo, const float* bias, int relu, double* gstat, int Cin, int M, int N,
                    int Hi, int Wi, int Ho, int Wo, int KH, int KW, int padh, int padw, int dtype, hipStream_t st) {
    OCRS_CHECK_ARG(x && wpk && out && Cin % 32 == 0 && ldx >= Cin && M > 0 && ldo >= M && ldo % 4 == 0 && KH >= 1 && KW >= 1 && KH * KW <= 9);
    if (conv3x3_tile_supported(ldx, ldo, Cin, M, Hi, Wi, Ho, Wo, KH, KW, padh, padw, dtype))  // narrow layers, weights resident in LDS (rec_conv4.hip)
        return conv3x3_tile_launch(x, ldx, wpk, out, ldo, bias, relu, gstat, Cin, M, N, Hi, Wi, st);
    if (conv3x3_rows_supported(ldx, ldo, Cin, M, Hi, Wi, Ho, Wo, KH, KW, padh, padw, dtype))  // whole-row passes, one workgroup per CU (rec_conv3.hip)
        return conv3x3_rows_launch(x, ldx, wpk, out, ldo, bias, relu, gstat, Cin, M, N, Hi, Wi, Ho, Wo, KW, padh, st);
    if (conv3x3_c128_supported(ldx, ldo, Cin, M, Hi, Wi, Ho, Wo, KH, KW, padh, padw, dtype))  // the 128-output-channel 3x3 layers: 128 x 256 block tiles (rec_conv2.hip)
        return conv3x3_c128_launch(x, ldx, wpk, out, ldo, bias, relu, gstat, Cin, N, Hi, Wi, st);
    const bool gemm = Ho == 1 && KH == 1;
    if (dtype == 1)
        return gemm ? launch_igemm<bf16, 1, 128>(x, ldx, wpk, out, ldo, bias, relu, gstat, Cin, M, N, Hi, Wi, Ho, Wo, KH, KW, padh, padw, st)
                    : launch_igemm<bf16, 8, 16>(x, ldx, wpk, out, ldo, bias, relu, gstat, Cin, M, N, Hi, Wi, Ho, Wo, KH, KW, padh, padw, st);
    return gemm ? launch_igemm<float, 1, 128>(x, ldx, wpk, out, ldo, bias, relu, gstat, Cin, M, N, Hi, Wi, Ho, Wo, KH, KW, padh, padw, st)
                : launch_igemm<float, 8, 16>(x, ldx, wpk, out, ldo, bias, relu, gstat, Cin, M, N, Hi, Wi, Ho, Wo, KH, KW, padh, padw, st);
}

}  // extern "C"
