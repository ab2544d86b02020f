// Detection U-Net forward kernels (gfx950).  Reference semantics: ocrs_models/models.py:7-143.
//
//  k_dwpw_fwd      fused [producer BN+ReLU on load] -> depthwise 3x3 -> pointwise 1x1 (MFMA) -> z + BN batch sums
//  k_bn_finalize   batch sums -> (scale, shift, lo) + saved mean/rstd + running-stat update
//  k_maxpool_fwd   2x2 max-pool of relu(bn(z))
// The first block, the ConvTranspose2d forward and the head have their own files (det_c1 / det_convt / det_head.hip).
#include "det_internal.h"

// ----------------------------------------------------------------------------------------------
// generic weight-fragment packer:  W[k][m]  ->  MFMA fragments [kc][mt][lane][8]
//   mode 0: element (k, m) at src[(k / K2) * s1 + (k % K2) * s2 + m * sm]
//   mode 1: ConvTranspose2d forward "effective" weight (src = W[Cup][Cout][3][3], K2 = Cup, M = 4*Cout):
//           k = d*Cup + c (d = dy*2+dx), m = q*Cout + o (q = py*2+px) -> W[c][o][py+2dy][px+2dx] or 0
//   mode 2 (bf16 only): mode-0 addressing, SPLIT into hi = bf16(w), lo = bf16(w - hi): [kc][mt][plane = hi, lo][lane][8] (twice the bytes
//           of a plain bf16 pack) -- the A operand of the split-bf16 GEMM k_gemm_x3p (rec_gemm.hip)
// ----------------------------------------------------------------------------------------------
template <class T>
__device__ __forceinline__ void pack_frags_body(const float* __restrict__ src, int mode, int K, int M, int K2, long s1, long s2, long sm, T* __restrict__ out,
                                                long idx) {
    const int MT = (M + 15) / 16;
    const int nkc = (K + 31) / 32;
    if (idx >= (long)nkc * MT * 64) return;
    const int lane = (int)(idx & 63);
    const long frag = idx >> 6;
    const int mt = (int)(frag % MT), kc = (int)(frag / MT);
    const int m = mt * 16 + (lane & 15);
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = Elem<T>::is_bf16 ? kc * 32 + (lane >> 4) * 8 + j : kc * 32 + j * 4 + (lane >> 4);
        float x = 0.f;
        if (k < K && m < M) {
            if (mode == 0 || mode == 2) {
                x = src[(long)(k / K2) * s1 + (long)(k % K2) * s2 + (long)m * sm];
            } else {
                const int Cup = K2, Cout = M / 4;
                const int d = k / Cup, c = k % Cup, q = m / Cout, o = m % Cout;
                const int ky = (q >> 1) + 2 * (d >> 1), kx = (q & 1) + 2 * (d & 1);
                if (ky < 3 && kx < 3) x = src[((long)c * Cout + o) * 9 + ky * 3 + kx];
            }
        }
        v[j] = x;
    }
    if constexpr (Elem<T>::is_bf16) {
        if (mode == 2) {
            float lo[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float h = Elem<bf16>::round(v[j]);
                lo[j] = v[j] - h;
                v[j] = h;
            }
            store8(out + ((frag * 2) * 64 + lane) * 8, v);
            store8(out + ((frag * 2 + 1) * 64 + lane) * 8, lo);
            return;
        }
    }
    store8(out + idx * 8, v);
}
template <class T>
__global__ void k_pack_frags(const float* __restrict__ src, int mode, int K, int M, int K2, long s1, long s2, long sm, T* __restrict__ out) {
    pack_frags_body<T>(src, mode, K, M, K2, s1, s2, sm, out, (long)blockIdx.x * blockDim.x + threadIdx.x);
}
// all weight packs of a train step in ONE launch (they were 74 launches x 4.4 us): blockIdx.y = table row
//   table [n][9] int64 = { src, out, mode, K, M, K2, s1, s2, sm }
template <class T>
__global__ void k_pack_frags_multi(const long long* __restrict__ table) {
    const long long* r = table + (long)blockIdx.y * 9;
    pack_frags_body<T>(reinterpret_cast<const float*>(r[0]), (int)r[2], (int)r[3], (int)r[4], (int)r[5], (long)r[6], (long)r[7], (long)r[8],
                       reinterpret_cast<T*>(r[1]), (long)blockIdx.x * blockDim.x + threadIdx.x);
}

// ----------------------------------------------------------------------------------------------
// fused depthwise+pointwise forward.
//   CG  = channel groups (of 8) per K-chunk = min(CIN,32)/8   -> tile = TP = PX*256/CG pixels, PX pixels x one group per thread
//   MT  = ceil(COUT/16) output-channel tiles, every wave computes all MT tiles for its 16*PTW pixels
// D[cout][pixel] = sum_cin Wpw[cout][cin] * u[pixel][cin],  u = dw3x3(x~)   (channels = MFMA M, pixels = MFMA N)
// so each lane ends up with 4 consecutive output channels of one pixel -> 8/16-byte NHWC stores.
// ----------------------------------------------------------------------------------------------
// Tile geometry: every thread computes the depthwise output of PX horizontally adjacent pixels for one group of 8 channels.
//   PX = 2 (COUT <= 64): the two pixels share 6 of their 9 taps and all 72 weights -> 12 + 9 LDS vector reads per pair instead of
//   2 x (9 + 9): the kernel is LDS-bandwidth bound at the top levels (SQ_LDS_IDX_ACTIVE 77 % of the kernel's cycles), this removes
//   ~40 % of that traffic.  Tiles: CG=1 16x32, CG=2 16x16, CG=4 8x16 pixels (PX = 1, COUT > 64: 8x32 / 8x16 / 8x8).
template <int CG, int PX>
struct FwdTile {
    static constexpr int TP = PX * 256 / CG;
    static constexpr int TW = (PX == 2 && CG == 4) ? 16 : 32 / CG;
    static constexpr int TH = TP / TW;
};
template <int MT>
struct FwdPx {
    static constexpr int PX = MT <= 4 ? 2 : 1;
};
// LDS pitch (elements) of the depthwise-output tile [TP][CG*8 + pad]: 16-byte aligned rows, conflict-free fragment reads
template <class T, int CG>
struct FwdPitch {
    static constexpr int V = CG * 8 + (Elem<T>::is_bf16 ? 8 : 4);
};

template <class T, int CG, int MT, bool ONE /* Cin == CG*8: a single K chunk (always true for CG < 4) */, bool POOL = false /* also write the 2x2 max-pool */>
__global__ __launch_bounds__(256, (ONE && Elem<T>::is_bf16) ? 3 : (MT <= 4 ? 4 : 2)) void k_dwpw_fwd(Src2<T> x, const float* __restrict__ tra, const float* __restrict__ trb,
                                                                    const float* __restrict__ wdw /*master [CIN][1][3][3]*/,
                                                                    const void* __restrict__ wpk, T* __restrict__ z,
                                                                    double* __restrict__ gstat /*[2][COUT]*/, int CIN, int COUT, Tiling2 tg,
                                                                    const float* __restrict__ gamma /*[COUT] or null*/,
                                                                    T* __restrict__ pooled /*[N][H/2][W/2][COUT] or null*/) {
    constexpr int PX = FwdPx<MT>::PX;
    using FT = FwdTile<CG, PX>;
    constexpr int TW = FT::TW, TH = FT::TH, TP = FT::TP;
    constexpr int PTW = TP / 64;
    constexpr int KS = CG * 2;  // fp32 k-steps (of 4) per chunk
    constexpr int PITCH = FwdPitch<T, CG>::V;
    constexpr int HP = HaloTile<TW, TH>::HP;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* tile = reinterpret_cast<T*>(smem);                                                   // [TP][PITCH]  dw output (MFMA operand)
    float* xs = reinterpret_cast<float*>(smem + ((TP * PITCH * sizeof(T) + 15) & ~15));     // 2 planes [HP*CG][4]: transformed input + halo
    float* s_par = xs + HP * CG * 8;                                                         // [12][CIN]: tr(3, HaloStager layout) | wdw(9, tap-major)
    float* s_stat = s_par + 12 * CIN;                                                        // [wave][2][MT*16]: one slot per wave, no atomics
    const int H = tg.H, W = tg.W;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    fill_tr8(s_par, x, tra, trb, CIN, tid);
    for (int i = tid; i < 9 * CIN; i += 256) {
        const int t = i / CIN, c = i - t * CIN;
        s_par[3 * CIN + i] = wdw[c * 9 + t];
    }
    for (int i = tid; i < 4 * 2 * MT * 16; i += 256) s_stat[i] = 0.f;
    __syncthreads();
    const HaloStager<T, CG, TW, TH> stager(tid, W);

    const int nkc = ONE ? 1 : CIN / (CG * 8);
    const int pgrp = tid / CG, cg = tid % CG;     // pixel (PX = 1) or pixel pair (PX = 2) of this thread
    const int ty = pgrp / (TW / PX), tx = (pgrp % (TW / PX)) * PX;
    const int pxl = ty * TW + tx;

    TileSched ts(tg.ntiles);
    constexpr bool PIPE = ONE && Elem<T>::is_bf16;  // single-chunk bf16 configs (Cin <= 32, levels 0-2): register-prefetch the next tile
    typename HaloStager<T, CG, TW, TH>::Pending pend;
    typename Mma<T>::Frag wfr[PIPE ? MT : 1];  // PIPE: pointwise weight fragments are tile-invariant -> registers (a global load inside
                                                // the loop would make the compiler wait vmcnt(0), i.e. for the prefetch as well)
    TileIter<TW, TH> tit(tg, ts.first < ts.end ? ts.first : 0, ts.step);  // PIPE: origin of the prefetched tile, no divisions in the loop
    TileOrg org_next = tit.org();
    if constexpr (PIPE) {
#pragma unroll
        for (int b = 0; b < MT; ++b) {
            wfr[b] = Mma<T>::load_w(wpk, (long)b, lane);
            // consume the load HERE: otherwise its first use inside the loop carries a vmcnt(0) (PIPE implies bf16: Frag = uint4)
            asm volatile("" : "+v"(wfr[b].q.x), "+v"(wfr[b].q.y), "+v"(wfr[b].q.z), "+v"(wfr[b].q.w));
        }
        if (ts.first < ts.end) stager.issue(pend, x, 0, org_next, H, W, tid);
    }
    for (long t = ts.first; t < ts.end; t += ts.step) {
        const TileOrg org = PIPE ? org_next : tile_origin2<TW, TH>(tg, (int)t);
        f32x4 acc[PTW][MT];
#pragma unroll
        for (int a = 0; a < PTW; ++a)
#pragma unroll
            for (int b = 0; b < MT; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};

        for (int kc = 0; kc < nkc; ++kc) {
            if constexpr (PIPE) {
                // this tile's input was issued one tile ago; transform it into LDS, then issue the next tile's loads so that
                // their HBM latency hides under the tap / MFMA / store phases below
                stager.commit(pend, s_par, 0, xs, tid);
                __builtin_amdgcn_sched_barrier(0);  // keep the next tile's loads behind ALL of this tile's commit waits
                if (t + ts.step < ts.end) {
                    tit.next();
                    org_next = tit.org();
                    stager.issue(pend, x, 0, org_next, H, W, tid);
                }
            } else
                stager.stage(x, s_par, kc * CG * 8, org, H, W, xs, tid);
            tile_barrier<PIPE>();  // xs ready; all readers of the previous xs / tile passed a barrier since
            if constexpr (PX == 2) {
                float u0[8], u1[8];
                dw2_from_lds<CG, TW, TH>(xs, s_par + 3 * CIN, CIN, (kc * CG + cg) * 8, cg, ty, tx, u0, u1);
                store8_opaque(tile + pxl * PITCH + cg * 8, u0);
                store8_opaque(tile + (pxl + 1) * PITCH + cg * 8, u1);
            } else {
                float u[8];
                dw_from_lds<CG, TW, TH>(xs, s_par + 3 * CIN, CIN, (kc * CG + cg) * 8, cg, ty, tx, u);
                store8_opaque(tile + pxl * PITCH + cg * 8, u);
            }
            tile_barrier<PIPE>();
            typename Mma<T>::Frag pf[PTW];
#pragma unroll
            for (int a = 0; a < PTW; ++a) pf[a] = Mma<T>::load_p(tile, PITCH, (wave * PTW + a) * 16, lane, CG * 8);
#pragma unroll
            for (int b = 0; b < MT; ++b) {
                typename Mma<T>::Frag wf;
                if constexpr (PIPE)
                    wf = wfr[b];
                else
                    wf = Mma<T>::load_w(wpk, (long)kc * MT + b, lane);
#pragma unroll
                for (int a = 0; a < PTW; ++a) acc[a][b] = Mma<T>::template mma<KS>(wf, pf[a], acc[a][b]);
            }
        }
        // epilogue: store z (4 consecutive channels per lane) + per-channel sum / sum of squares
        const long tile_base = ((long)org.n * H + org.h0) * W + org.w0;
#pragma unroll
        for (int b = 0; b < MT; ++b) {
            const int m0 = b * 16 + (lane >> 4) * 4;
            float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int a = 0; a < PTW; ++a) {
                const int q = (wave * PTW + a) * 16 + (lane & 15);  // output pixel of this lane (MFMA N index)
                const int oty = q / TW, otx = q % TW;
                const bool ov = org.h0 + oty < H && org.w0 + otx < W;
                if (ov && m0 < COUT) {
                    const f32x4 v = acc[a][b];
                    store4(z + (tile_base + (long)oty * W + otx) * COUT + m0, v[0], v[1], v[2], v[3]);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float qv = Elem<T>::round(v[r]);  // statistics of what the consumer will read
                        s1[r] += qv;
                        s2[r] = fmaf(qv, qv, s2[r]);
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float a1 = quad16_sum(s1[r]), a2 = quad16_sum(s2[r]);
                if ((lane & 15) == 0) {  // the only lane of this wave that owns channel m0 + r: plain read-modify-write of the wave's slot
                    s_stat[wave * 2 * MT * 16 + m0 + r] += a1;
                    s_stat[wave * 2 * MT * 16 + MT * 16 + m0 + r] += a2;
                }
            }
            // ---- fused MaxPool2d(2) (models.py:54) in its pre-BatchNorm form: the consumer sees relu(bn(z)), monotone in z with the sign of
            // gamma (known before the batch statistics are), so the window's selected element is max z (gamma >= 0) or min z (gamma < 0); its z
            // is written to `pooled` and read through this block's load transform like any block output (see k_maxpool_fwd<T, true>, which
            // this replaces at levels 0-2: the full-size z is not read again).  A 2x2 window = this lane's pixel, the next lane's (same row:
            // an N tile is 16 consecutive pixels of a tile row) and the same two lanes of the N tile one row below (same wave: rows per
            // wave are even).  Ties between different z can only differ from k_maxpool_fwd's first-maximum rule where bn(z) rounds to the
            // same value; the selected VALUE, which is all consumers see, then differs by that rounding.
            if constexpr (POOL && PX == 2 && TW >= 16) {
                {
                    constexpr int TPR = TW / 16;
                    float sg[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) sg[r] = (m0 + r < COUT && gamma[m0 + r] < 0.f) ? -1.f : 1.f;
                    const int Hp = H >> 1, Wp = W >> 1;
#pragma unroll
                    for (int a = 0; a < PTW; ++a) {
                        const int q = (wave * PTW + a) * 16 + (lane & 15);
                        const int oty = q / TW, otx = q % TW;
                        if ((oty & 1) == 0) {  // (compile-time after unrolling: a / TPR is the row within the wave)
                            float m4[4];
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const float v0 = sg[r] * Elem<T>::round(acc[a][b][r]), v1 = sg[r] * Elem<T>::round(acc[a + TPR][b][r]);
                                const float vv = fmaxf(v0, v1);
                                m4[r] = sg[r] * fmaxf(vv, dpp_f<0xB1>(vv));  // quad_perm [1,0,3,2]: the horizontally adjacent pixel (lane ^ 1), no LDS
                            }
                            const int ph = (org.h0 + oty) >> 1, pw = (org.w0 + otx) >> 1;
                            if ((lane & 1) == 0 && ph < Hp && pw < Wp && m0 < COUT)
                                store4(pooled + (((long)org.n * Hp + ph) * Wp + pw) * COUT + m0, m4[0], m4[1], m4[2], m4[3]);
                        }
                    }
                }
            }
        }
    }
    __syncthreads();
    for (int c = tid; c < COUT; c += 256) {
        constexpr int WS = 2 * MT * 16;
        atomicAdd(&gstat[c], (double)((s_stat[c] + s_stat[WS + c]) + (s_stat[2 * WS + c] + s_stat[3 * WS + c])));
        atomicAdd(&gstat[COUT + c], (double)((s_stat[MT * 16 + c] + s_stat[WS + MT * 16 + c]) + (s_stat[2 * WS + MT * 16 + c] + s_stat[3 * WS + MT * 16 + c])));
    }
}

// BatchNorm2d training-mode statistics (biased var for normalisation, unbiased into running_var, eps 1e-5,
// momentum 0.1)  ->  per-channel load transform + saved mean/rstd.
__global__ void k_bn_finalize(const double* __restrict__ gstat, long count, int C, const float* __restrict__ gamma,
                              const float* __restrict__ beta, float eps, float momentum, float* __restrict__ tr /*[3][C]*/,
                              float* __restrict__ saved /*[2][C] mean|rstd*/, float* __restrict__ run_mean, float* __restrict__ run_var,
                              long long* __restrict__ nbt, float lo) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c == 0 && nbt) *nbt += 1;
    if (c >= C) return;
    const double mean = gstat[c] / (double)count;
    double var = gstat[C + c] / (double)count - mean * mean;
    if (var < 0) var = 0;
    const float rstd = (float)(1.0 / sqrt(var + (double)eps));
    const float sc = gamma[c] * rstd;
    tr[c] = sc;
    tr[C + c] = beta[c] - (float)mean * sc;
    tr[2 * C + c] = lo;
    saved[c] = (float)mean;
    saved[C + c] = rstd;
    if (run_mean) {
        const double unb = count > 1 ? var * (double)count / (double)(count - 1) : var;
        run_mean[c] = (1.f - momentum) * run_mean[c] + momentum * (float)mean;
        run_var[c] = (1.f - momentum) * run_var[c] + momentum * (float)unb;
    }
}

// MaxPool2d(2) (models.py:54) over relu(bn(z)); floor output size.
// RAW = false: out = max over the window of act(z).  RAW = true: out = the PRE-BatchNorm z of the element with the largest act(z) (first
// one on ties), so that the pooled tensor is consumed exactly like a block output (consumers apply the producer's load transform, which
// reproduces act(z_sel) = the max bit for bit) and the depthwise-backward passes that read it can produce the producer's
// BatchNorm-backward sums (the gradient only lands on the selected elements) -- no separate bn_bwd_reduce pass over the full-size z.
template <class T, bool RAW>
__global__ __launch_bounds__(256) void k_maxpool_fwd(const T* __restrict__ z, const float* __restrict__ tr, T* __restrict__ out, int C, int H,
                                                     int W, long Pp) {
    const int CG = C / 8;
    const int Hp = H >> 1, Wp = W >> 1;
    const long total = Pp * CG;
    for (long it = (long)blockIdx.x * 256 + threadIdx.x; it < total; it += (long)gridDim.x * 256) {
        const long pp = it / CG;
        const int c0 = (int)(it - pp * CG) * 8;
        const PixIdx q = decode_pixel(pp, Hp, Wp);
        const long base = ((long)q.n * H + 2 * q.h) * W + 2 * q.w;
        float m[8], zr[8];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float v[8], a[8];
            load8(z + (base + (long)(k >> 1) * W + (k & 1)) * C + c0, v);
#pragma unroll
            for (int i = 0; i < 8; ++i) a[i] = v[i];
            apply_tr8(a, tr, C, c0);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                if (k == 0 || a[i] > m[i]) {
                    m[i] = a[i];
                    zr[i] = v[i];
                }
            }
        }
        if (RAW) store8(out + pp * C + c0, zr);
        else store8(out + pp * C + c0, m);
    }
}

// ----------------------------------------------------------------------------------------------
// host side
// ----------------------------------------------------------------------------------------------
template <class T, int CG, int MT, bool ONE>
static int launch_dwpw_fwd(const void* xa, const void* xb, int Ca, int Cb, const float* tra, const float* trb, const float* wdw, const void* wpk, void* z,
                           double* gstat, int COUT, int N, int H, int W, const float* gamma, void* pooled, hipStream_t st) {
    using FT = FwdTile<CG, FwdPx<MT>::PX>;
    constexpr int TP = FT::TP;
    const int CIN = Ca + Cb;
    Src2<T> x{(const T*)xa, (const T*)xb, Ca, Cb};
    const Tiling2 tg = make_tiling2(N, H, W, FT::TW, FT::TH);
    const size_t smem = ((TP * FwdPitch<T, CG>::V * sizeof(T) + 15) & ~15) +
                        (HaloTile<FT::TW, FT::TH>::HP * CG * 8 + 12 * CIN + 4 * 2 * MT * 16) * sizeof(float);
    // every block ends with 2*COUT same-address fp64 atomics (~15 ns each, serialised): at the middle levels (a few thousand tiles)
    // two tiles per block halve that tail; below that parallelism matters more (measured: tiles-per-block sweep, profiles/README.md)
    const int tpb = tg.ntiles >= 2048 ? 2 : 1;
    // 4 blocks per CU are resident (registers <= 128, LDS 36 KB): a grid of exactly the resident blocks runs as ONE round (8 per CU = two rounds, each
    // block with its own prologue and 2*COUT fp64 atomics at the end: 4.66 -> 4.52 ms per step over all forward launches)
    const int grid = persistent_grid(tg.ntiles / tpb > 0 ? tg.ntiles / tpb : 1, 4);
    if (pooled) {
        if constexpr (FwdPx<MT>::PX == 2 && FT::TW >= 16)
            hipLaunchKernelGGL((k_dwpw_fwd<T, CG, MT, ONE, true>), dim3(grid), dim3(256), smem, st, x, tra, trb, wdw, wpk, (T*)z, gstat, CIN, COUT, tg,
                               gamma, (T*)pooled);
        else
            return OCRS_ERR_ARG;  // (ocrs_dwpw_fwd_pool_supported)
    } else
        hipLaunchKernelGGL((k_dwpw_fwd<T, CG, MT, ONE, false>), dim3(grid), dim3(256), smem, st, x, tra, trb, wdw, wpk, (T*)z, gstat, CIN, COUT, tg,
                           gamma, (T*)pooled);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

template <class T>
static int dispatch_dwpw_fwd(const void* xa, const void* xb, int Ca, int Cb, const float* tra, const float* trb, const float* wdw, const void* wpk, void* z,
                             double* gstat, int COUT, int N, int H, int W, const float* gamma, void* pooled, hipStream_t st) {
    const int CIN = Ca + Cb;
    const int cg = CIN >= 32 ? 4 : CIN / 8;
    const int mt = (COUT + 15) / 16;
#define DWPW_CASE(CG_, MT_, ONE_) \
    if (cg == CG_ && mt == MT_ && (CIN == CG_ * 8) == ONE_) \
        return launch_dwpw_fwd<T, CG_, MT_, ONE_>(xa, xb, Ca, Cb, tra, trb, wdw, wpk, z, gstat, COUT, N, H, W, gamma, pooled, st);
    DWPW_CASE(1, 1, true) DWPW_CASE(2, 1, true) DWPW_CASE(2, 2, true)
    DWPW_CASE(4, 1, true) DWPW_CASE(4, 2, true) DWPW_CASE(4, 4, true)  // Cin == 32: pipelined single-chunk variants
    DWPW_CASE(4, 1, false) DWPW_CASE(4, 2, false) DWPW_CASE(4, 4, false) DWPW_CASE(4, 8, false) DWPW_CASE(4, 16, false)
#undef DWPW_CASE
    return OCRS_ERR_ARG;
}

// ----------------------------------------------------------------------------------------------
// C ABI
// ----------------------------------------------------------------------------------------------
extern "C" {

int ocrs_pack_frags(const float* src, int mode, int K, int M, int K2, long s1, long s2, long sm, void* out, int dtype, hipStream_t st) {
    OCRS_CHECK_ARG(src && out && K > 0 && M > 0 && K2 > 0);
    const long n = (long)((K + 31) / 32) * ((M + 15) / 16) * 64;
    const int grid = (int)((n + 255) / 256);
    if (dtype == 1)
        hipLaunchKernelGGL(k_pack_frags<bf16>, dim3(grid), dim3(256), 0, st, src, mode, K, M, K2, s1, s2, sm, (bf16*)out);
    else
        hipLaunchKernelGGL(k_pack_frags<float>, dim3(grid), dim3(256), 0, st, src, mode, K, M, K2, s1, s2, sm, (float*)out);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

// table: device int64 [n][9] = { src ptr, out ptr, mode, K, M, K2, s1, s2, sm } (the arguments of ocrs_pack_frags per row);
// max_frag_threads = max over rows of ceil(K/32) * ceil(M/16) * 64.
int ocrs_pack_frags_multi(const long long* table, int n, long max_frag_threads, int dtype, hipStream_t st) {
    OCRS_CHECK_ARG(table && n > 0 && max_frag_threads > 0);
    const dim3 grid((unsigned)((max_frag_threads + 255) / 256), (unsigned)n);
    if (dtype == 1)
        hipLaunchKernelGGL(k_pack_frags_multi<bf16>, grid, dim3(256), 0, st, table);
    else
        hipLaunchKernelGGL(k_pack_frags_multi<float>, grid, dim3(256), 0, st, table);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

// number of bytes a packed fragment buffer needs
long ocrs_pack_frags_bytes(int K, int M, int dtype) { return (long)((K + 31) / 32) * ((M + 15) / 16) * 64 * 8 * (dtype == 1 ? 2 : 4); }

// Fused DepthwiseConv block forward up to the pre-BatchNorm output (reference: ocrs_models/models.py:11-23).
//   xa/xb : NHWC inputs (xb may be null; channel concat [xa | xb] as torch.cat at models.py:89), Ca, Cb multiples of 8
//   tra/trb : [3][Ca] / [3][Cb] load transforms of the inputs (producer BN+ReLU, or identity)
//   wdw   : depthwise weights in the reference layout [Cin][1][3][3]; wpk: pointwise weights packed by ocrs_pack_frags(K=Cin, M=Cout)
//   z     : [P][Cout] pre-BN output; gstat: [2][Cout] double, sum z and sum z^2 ACCUMULATED (the caller zeroes it: one
//           memset for all layers of a step instead of one per launch)
// 1 if ocrs_dwpw_fwd can also write the 2x2-max-pooled (pre-BatchNorm) output: two-pixel tile configurations, Cout <= 64
long ocrs_dwpw_fwd_pool_supported(int Cin, int Cout) {
    if (det_dwf_supported(Cin, Cout, 1)) return 0;  // (the deep-level kernel is faster than the fusion saves: the max-pool stays its own pass there)
    return Cout <= 64 && (Cin < 32 || Cin % 32 == 0) ? 1 : 0;
}

//   gamma / pooled (nullable, need ocrs_dwpw_fwd_pool_supported): also write MaxPool2d(2) of the block output in its pre-BatchNorm form
//           (the selected element's z, chosen by the sign of the BatchNorm weight gamma [Cout]) to pooled [N][H/2][W/2][Cout]
int ocrs_dwpw_fwd(const void* xa, const void* xb, int Ca, int Cb, const float* tra, const float* trb, const float* wdw, const void* wpk,
                  void* z, double* gstat, const float* gamma, void* pooled, int Cout, int N, int H, int W, int dtype, hipStream_t st) {
    const int Cin = Ca + Cb;
    OCRS_CHECK_ARG(!pooled || (gamma && ocrs_dwpw_fwd_pool_supported(Cin, Cout)));
    OCRS_CHECK_ARG(xa && tra && wdw && wpk && z && gstat && (Cb == 0 || trb));
    OCRS_CHECK_ARG(Ca % 8 == 0 && Cb % 8 == 0 && Cin >= 8 && (Cin < 32 || Cin % 32 == 0) && Cout % 8 == 0 && Cout <= 256);
    OCRS_CHECK_ARG((Cb == 0) == (xb == nullptr));
    OCRS_CHECK_ARG((long)N * H * W < (1L << 31));
    if (!pooled && det_dwf_supported(Cin, Cout, dtype))
        return det_dwf_launch(xa, xb, Ca, Cb, tra, trb, wdw, wpk, z, gstat, Cout, N, H, W, st, FwdFin{nullptr, 0, nullptr, nullptr, 0.f, 0.f, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f});
    return dtype == 1 ? dispatch_dwpw_fwd<bf16>(xa, xb, Ca, Cb, tra, trb, wdw, wpk, z, gstat, Cout, N, H, W, gamma, pooled, st)
                      : dispatch_dwpw_fwd<float>(xa, xb, Ca, Cb, tra, trb, wdw, wpk, z, gstat, Cout, N, H, W, gamma, pooled, st);
}

// ocrs_dwpw_fwd + ocrs_bn_finalize in one launch (the deep-level forward kernel, det_dwf.hip: ocrs_dwpw_fwd_fin_supported): the last workgroup done
// finalises the BatchNorm statistics -- counter: a zeroed device word (left zeroed); count, bn_w .. lo: as ocrs_bn_finalize.  No pooling.
long ocrs_dwpw_fwd_fin_supported(int Cin, int Cout, int dtype) { return det_dwf_supported(Cin, Cout, dtype); }
int ocrs_dwpw_fwd_fin(const void* xa, const void* xb, int Ca, int Cb, const float* tra, const float* trb, const float* wdw, const void* wpk, void* z,
                      double* gstat, unsigned* counter, long count, const float* bn_w, const float* bn_b, float eps, float momentum, float* tr, float* saved,
                      float* run_mean, float* run_var, long long* nbt, float lo, int Cout, int N, int H, int W, int dtype, hipStream_t st) {
    const int Cin = Ca + Cb;
    OCRS_CHECK_ARG(xa && tra && wdw && wpk && z && gstat && (Cb == 0 || trb) && (Cb == 0) == (xb == nullptr));
    OCRS_CHECK_ARG(counter && count > 0 && bn_w && bn_b && tr && saved && ocrs_dwpw_fwd_fin_supported(Cin, Cout, dtype) && (long)N * H * W < (1L << 31));
    return det_dwf_launch(xa, xb, Ca, Cb, tra, trb, wdw, wpk, z, gstat, Cout, N, H, W, st,
                          FwdFin{counter, count, bn_w, bn_b, eps, momentum, tr, saved, run_mean, run_var, nbt, lo});
}

// BatchNorm2d batch statistics -> load transform (reference: nn.BatchNorm2d at models.py:23, training mode).
int ocrs_bn_finalize(const double* gstat, long count, int C, const float* gamma, const float* beta, float eps, float momentum, float* tr,
                     float* saved, float* run_mean, float* run_var, long long* nbt, float lo, hipStream_t st) {
    OCRS_CHECK_ARG(gstat && gamma && beta && tr && saved && C > 0 && count > 0);
    hipLaunchKernelGGL(k_bn_finalize, dim3((C + 63) / 64), dim3(64), 0, st, gstat, count, C, gamma, beta, eps, momentum, tr, saved, run_mean,
                       run_var, nbt, lo);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

// MaxPool2d(2) over relu(bn(z))  (models.py:54).  out: [N][H/2][W/2][C]; raw = 1: the selected elements' pre-BatchNorm z instead of the max
int ocrs_maxpool_fwd(const void* z, const float* tr, void* out, int C, int N, int H, int W, int raw, int dtype, hipStream_t st) {
    OCRS_CHECK_ARG(z && tr && out && C % 8 == 0 && H >= 2 && W >= 2 && (raw == 0 || raw == 1));
    const long Pp = (long)N * (H / 2) * (W / 2);
    const int grid = ew_grid(Pp * (C / 8));
#define OCRS_POOL(T_, R_) hipLaunchKernelGGL((k_maxpool_fwd<T_, R_>), dim3(grid), dim3(256), 0, st, (const T_*)z, tr, (T_*)out, C, H, W, Pp)
    if (dtype == 1) {
        if (raw) OCRS_POOL(bf16, true);
        else OCRS_POOL(bf16, false);
    } else {
        if (raw) OCRS_POOL(float, true);
        else OCRS_POOL(float, false);
    }
#undef OCRS_POOL
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

}  // extern "C"
