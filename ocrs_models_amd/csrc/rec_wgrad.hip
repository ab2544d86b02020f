// Weight-gradient kernels of the CRNN recogniser (gfx950).  Reference: the autograd of ocrs_models/models.py:179-251.  K = positions in all of them;
// every kernel can flush per-block partials to a workspace that a reduce kernel sums in a fixed order (bit-reproducible), or -- workspace null --
// add into dW with float atomics.
//
//  k_wgrad_gather       gathered form for any kernel size / stride: D[rowch][(tap, colch)] = sum_pos A[pos][rowch] * B[pos*stride + tap - pad][colch]
//                       (Conv2d with A = dz, ConvTranspose2d, Linear, GRU); transposed, swizzled LDS tiles.  fp32, and bf16 without a workspace
//  k_wgrad_gather_tr    the same for bf16 with a workspace: natural-layout tiles + LDS transpose read
//  k_conv3x3_wgrad      3x3 / stride 1 / pad 1 with full operand reuse: all nine taps per staged tile (fp32)
//  k_conv3x3_wgrad_tr   its bf16 form on the LDS transpose read
//  k_wgrad_gemm_x3      split-bf16 GEMM for the fp32 GRU / Linear weight gradients (throughput mode)
//  k_wgrad_gather_reduce / k_wgrad3x3_reduce    fixed-order sums of the workspace partials into dW
#include "rec_internal.h"

// ---------------------------------------------------------------------------------------------------------------------
// D[ra][(tap, cb)] += sum_pos A~[pos][ra] * B[bpos(pos, tap)][cb];  A grid (N, hA, wA), B grid (N, HB, WB),
// bpos = (i*stride + ky - padh, j*stride + kx - padw).  Block = (<=128 A channels) x (128 columns (tap, cb)); K = positions.
// dW index = (ra * CB + cb) * ntaps + tap  (covers Conv2d [Cout][Cin][kh][kw] with A = dz, and ConvTranspose2d / Linear / GRU).
// LDS tiles are stored transposed ([channel][pixel], pixel = MFMA K) with the 8-pixel column blocks XOR-swizzled by
// (row >> 3) & 7: with 16-byte-aligned rows every 8th row would otherwise start on the same bank (16-way conflicts on the
// scalar transposed stores); lanes are mapped pixel-fastest so 16 lanes write 16 consecutive pixels of one channel.
template <class T>
__device__ __forceinline__ typename Mma<T>::Frag load_swz(const T* tile, int tpp, int row0, int pc, int lane);
template <>
__device__ __forceinline__ Mma<bf16>::Frag load_swz<bf16>(const bf16* tile, int tpp, int row0, int pc, int lane) {
    const int row = row0 + (lane & 15);
    const int blk = (pc * 4 + (lane >> 4)) ^ ((row >> 3) & 7);
    Mma<bf16>::Frag f;
    f.q = *reinterpret_cast<const uint4*>(tile + row * tpp + blk * 8);
    return f;
}
template <>
__device__ __forceinline__ Mma<float>::Frag load_swz<float>(const float* tile, int tpp, int row0, int pc, int lane) {
    const int row = row0 + (lane & 15);
    const int sw = (row >> 3) & 7;
    Mma<float>::Frag f;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
        const int px = pc * 32 + ks * 4 + (lane >> 4);
        f.v[ks] = tile[row * tpp + (((px >> 3) ^ sw) << 3) + (px & 7)];
    }
    return f;
}

// store the same channel of two adjacent pixels (px even) as one LDS word / pair
__device__ __forceinline__ void st_pair(bf16* dst, float a, float b) { *reinterpret_cast<unsigned*>(dst) = pack2bf(a, b); }
__device__ __forceinline__ void st_pair(float* dst, float a, float b) { *reinterpret_cast<float2*>(dst) = make_float2(a, b); }

// TP pixels per tile (128 for bf16, 64 for fp32: LDS).  Software-pipelined: the raw global loads of tile t+1 are issued before the
// MFMA phase of tile t (the kernel runs at one block per CU, so nothing else would hide the HBM latency).
template <class T, int TP>
__global__ __launch_bounds__(256) void k_wgrad_gather(const T* __restrict__ A, int ldA, int CA, const float* __restrict__ trA, const T* __restrict__ B,
                                                      int ldB, int CB, float* __restrict__ dW, int N, int hA, int wA, int HB, int WB, int stride,
                                                      int padh, int padw, int KH, int KW, float* __restrict__ ws) {
    constexpr int TPP = Elem<T>::is_bf16 ? TP + 8 : TP + 4;
    constexpr int NPB = TP / 64;       // 64-pixel blocks per tile (swizzle works inside a 64-pixel block)
    constexpr int NIT = TP / 32;       // (pixel pair, group) items per thread, A side (max) and B side
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* aT = reinterpret_cast<T*>(smem);  // [128][TPP]
    T* bT = aT + 128 * TPP;              // [128][TPP]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int CA8 = (CA + 7) & ~7;
    const int nbi = (CA8 + 127) / 128;
    const int ci_base = (blockIdx.y % nbi) * 128;
    const int j_base = (blockIdx.y / nbi) * 128;
    const int ntaps = KH * KW;
    const int J = ntaps * CB;
    const int rows_here = (CA8 - ci_base) < 128 ? (CA8 - ci_base) : 128;
    const int NGA = rows_here / 8;
    const int NG4 = (NGA + 3) / 4;
    const int WTI = (rows_here + 15) / 16;
    const long P = (long)N * hA * wA;
    const long ntiles = (P + TP - 1) / TP;
    {
        const float zero8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int i = tid * 8; i < 256 * TPP; i += 256 * 8) store8(aT + i, zero8);
    }
    // work items: (pixel PAIR, 8-channel group); lanes = 4 groups x 16 pairs per wave -> 64-byte global segments per pixel,
    // 32-bit LDS stores (two pixels of one channel).  A: item j of this thread = (group gA[j], pair ppA[j]); B: fixed column group.
    const int g4 = tid & 3, pp16 = (tid >> 2) & 15, blk = tid >> 6;
    const int jjB = (blk * 4 + g4) * 8;
    const int j0B = j_base + jjB;
    const bool colB = j0B < J;
    const int tapB = colB ? j0B / CB : 0, c0B = j0B - tapB * CB;
    const int dyB = tapB / KW - padh, dxB = tapB % KW - padw;

    Raw8<T> ra[NIT][2], rb[NIT][2];
    unsigned oka = 0, okb = 0;
    auto issue = [&](long t) {
        const long p0 = t * TP;
        oka = okb = 0;
#pragma unroll
        for (int j = 0; j < NIT; ++j) {
            const int it = tid + 256 * j;
            const int grp = g4 + 4 * ((it >> 6) % NG4), pp = pp16 + 16 * ((it >> 6) / NG4);
            if (grp < NGA && pp < TP / 2) {
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const long p = p0 + 2 * pp + e;
                    if (p < P) {
                        ra[j][e] = load8_raw(A + p * ldA + ci_base + grp * 8);
                        oka |= 1u << (2 * j + e);
                    }
                }
            }
        }
        const PixIdx base = decode_pixel(p0 < P ? p0 : 0, hA, wA);
#pragma unroll
        for (int j = 0; j < NIT; ++j) {
            const int pp = pp16 + 16 * j;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int off = 2 * pp + e;
                if (colB && p0 + off < P) {
                    int w = base.w + off, h = base.h, n = base.n;
                    while (w >= wA) {
                        w -= wA;
                        if (++h >= hA) {
                            h = 0;
                            ++n;
                        }
                    }
                    const int Y = h * stride + dyB, X = w * stride + dxB;
                    if (Y >= 0 && Y < HB && X >= 0 && X < WB) {
                        rb[j][e] = load8_raw(B + (((long)n * HB + Y) * WB + X) * ldB + c0B);
                        okb |= 1u << (2 * j + e);
                    }
                }
            }
        }
    };
    auto commit = [&]() {
#pragma unroll
        for (int j = 0; j < NIT; ++j) {
            const int it = tid + 256 * j;
            const int grp = g4 + 4 * ((it >> 6) % NG4), pp = pp16 + 16 * ((it >> 6) / NG4);
            if (grp < NGA && pp < TP / 2) {
                const int c0 = grp * 8;
                float v[2][8];
#pragma unroll
                for (int e = 0; e < 2; ++e) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) v[e][i] = 0.f;
                    if (oka & (1u << (2 * j + e))) {
                        unpack8(ra[j][e], v[e]);
                        if (trA) apply_tr8(v[e], trA, CA, ci_base + c0);
                    }
                }
                const int px = 2 * pp, pb = px >> 6, pl = px & 63;
                T* dst = aT + c0 * TPP + pb * 64 + ((((pl >> 3) ^ ((c0 >> 3) & 7)) << 3) | (pl & 7));
#pragma unroll
                for (int i = 0; i < 8; ++i) st_pair(dst + i * TPP, v[0][i], v[1][i]);
            }
        }
#pragma unroll
        for (int j = 0; j < NIT; ++j) {
            const int pp = pp16 + 16 * j;
            float v[2][8];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
#pragma unroll
                for (int i = 0; i < 8; ++i) v[e][i] = 0.f;
                if (okb & (1u << (2 * j + e))) unpack8(rb[j][e], v[e]);
            }
            const int px = 2 * pp, pb = px >> 6, pl = px & 63;
            T* dst = bT + jjB * TPP + pb * 64 + ((((pl >> 3) ^ ((jjB >> 3) & 7)) << 3) | (pl & 7));
#pragma unroll
            for (int i = 0; i < 8; ++i) st_pair(dst + i * TPP, v[0][i], v[1][i]);
        }
    };

    f32x4 acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    TileSched ts(ntiles);
    if (ts.first < ts.end) issue(ts.first);
    __syncthreads();
    for (long t = ts.first; t < ts.end; t += ts.step) {
        commit();
        __syncthreads();
        if (t + ts.step < ts.end) issue(t + ts.step);  // in flight during the MFMA phase
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int tt = wave + 4 * j;
            if (tt < WTI * 8) {
                const int ti = tt % WTI, tj = tt / WTI;
#pragma unroll
                for (int pb = 0; pb < NPB; ++pb)
#pragma unroll
                    for (int pc = 0; pc < 2; ++pc) {
                        const typename Mma<T>::Frag fa = load_swz<T>(aT + pb * 64, TPP, ti * 16, pc, lane);
                        const typename Mma<T>::Frag fb = load_swz<T>(bT + pb * 64, TPP, tj * 16, pc, lane);
                        acc[j] = Mma<T>::template mma<8>(fa, fb, acc[j]);
                    }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int tt = wave + 4 * j;
        if (tt < WTI * 8) {
            const int ti = tt % WTI, tj = tt / WTI;
            const int jc = j_base + tj * 16 + (lane & 15);
            if (jc < J) {
                const int ra0 = ci_base + ti * 16 + (lane >> 4) * 4;
                if (ws) {
                    // two-stage atomic-free flush: ws[blockIdx.x][jc][ra] (4 consecutive rows per lane = one 16-byte store)
                    if (ra0 < CA8)
                        *reinterpret_cast<float4*>(ws + ((long)blockIdx.x * J + jc) * CA8 + ra0) = make_float4(acc[j][0], acc[j][1], acc[j][2], acc[j][3]);
                } else {
                    const int tap = jc / CB, cb = jc - tap * CB;
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (ra0 + r < CA) atomicAdd(&dW[((long)(ra0 + r) * CB + cb) * ntaps + tap], acc[j][r]);
                }
            }
        }
    }
}

// dW[(ra*CB + cb)*ntaps + tap] += sum_bx ws[bx][jc = tap*CB + cb][ra];  grid ceil(n / 32), n = ntaps * CB * CA8 (det_column_sum: 32 elements x
// 8 interleaved chains per block, eight loads in flight per chain -- one thread per element walking its gx partials in turn was a pure
// latency chain: 15-60 us per launch for a few MB)
__global__ __launch_bounds__(256) void k_wgrad_gather_reduce(const float* __restrict__ ws, int gx, int CA, int CA8, int CB, int ntaps,
                                                             float* __restrict__ dW) {
    const long n = (long)ntaps * CB * CA8;
    const long i = (long)blockIdx.x * 32 + (threadIdx.x & 31);
    const int ra = (int)(i % CA8);
    float s;
    if (!det_column_sum(ws, gx, n, (i < n && ra < CA) ? i : n, s)) return;
    const long jc = i / CA8;
    const int tap = (int)(jc / CB), cb = (int)(jc - (long)tap * CB);
    dW[((long)ra * CB + cb) * ntaps + tap] += s;
}

// ---------------------------------------------------------------------------------------------------------------------
// Conv2d 3x3 / stride 1 / pad 1 weight gradient with full operand reuse:
//   dW[co][ci][ky][kx] += sum_{n,h,w} dz[n][h][w][co] * x[n][h+ky-1][w+kx-1][ci]
// Block = 8x16 pixel tile x 128 output channels x one 32-channel slice of Cin (grid.y) x ALL 9 taps:
//   dzT [128 co][128 px]                         (swizzled, staged once per tile)
//   xT  [3 kx][32 ci][10 halo rows x 16 px]      three column-shifted copies of the transposed input halo, so the B fragment of
//                                                 tap (ky,kx) is an ALIGNED 8-pixel read at row offset ky -- no per-tap re-staging.
// D[co][(tap, ci32)] = 8 x 18 MFMA tiles = 36 per wave (144 accumulator registers), K = 128 pixels per tile.
template <class T>
__global__ __launch_bounds__(256) void k_conv3x3_wgrad(const T* __restrict__ dz, int Cout, const T* __restrict__ x, int Cin, float* __restrict__ dW, int N,
                                                       int H, int W, float* __restrict__ ws) {
    constexpr int TH = 8, TW = 16, TP = 128;
    constexpr int DPP = Elem<T>::is_bf16 ? TP + 8 : TP + 4;  // dzT pitch
    constexpr int XR = 10 * 16;                                // pixels of one shifted halo image
    constexpr int XPP = Elem<T>::is_bf16 ? XR + 8 : XR + 4;   // xT pitch
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* dzT = reinterpret_cast<T*>(smem);   // [128][DPP]
    T* xT = dzT + 128 * DPP;               // [3][32][XPP]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ci_base = blockIdx.y * 32;
    const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
    const int ntiles = N * tiles_x * tiles_y;
    const int g4 = tid & 3, pp16 = (tid >> 2) & 15, blk = tid >> 6;
    f32x4 acc[36];
#pragma unroll
    for (int j = 0; j < 36; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    TileSched ts(ntiles);
    for (long t = ts.first; t < ts.end; t += ts.step) {
        const int tpi = tiles_x * tiles_y;
        const int n = (int)t / tpi, r = (int)t - n * tpi;
        const int h0 = (r / tiles_x) * TH, w0 = (r % tiles_x) * TW;
        __syncthreads();  // previous tile's fragment reads are done
        // ---- dzT: (pixel pair along w, 8-channel group) items: 64 pairs x 16 groups = 1024 -> 4 per thread
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int grp = g4 + 4 * blk, pp = pp16 + 16 * j;   // grp 0..15, pp 0..63 (pixel pair index: ty = pp / 8, tx = 2*(pp % 8))
            const int ty = pp >> 3, tx = (pp & 7) * 2;
            float v[2][8];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
#pragma unroll
                for (int i = 0; i < 8; ++i) v[e][i] = 0.f;
                const int h = h0 + ty, w = w0 + tx + e;
                if (h < H && w < W && grp * 8 < Cout) load8(dz + (((long)n * H + h) * W + w) * Cout + grp * 8, v[e]);
            }
            const int px = ty * 16 + tx, pb = px >> 6, pl = px & 63;
            T* dst = dzT + grp * 8 * DPP + pb * 64 + ((((pl >> 3) ^ (grp & 7)) << 3) | (pl & 7));
#pragma unroll
            for (int i = 0; i < 8; ++i) st_pair(dst + i * DPP, v[0][i], v[1][i]);
        }
        // ---- xT: wave = 8-channel group, lanes walk the 10x18 halo pixels; each pixel goes into the (up to) three shifted copies
        for (int hp = lane; hp < 10 * 18; hp += 64) {
            const int hy = hp / 18, hx = hp - hy * 18;
            const int h = h0 + hy - 1, w = w0 + hx - 1;
            float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (h >= 0 && h < H && w >= 0 && w < W) load8(x + (((long)n * H + h) * W + w) * Cin + ci_base + wave * 8, v);
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int tx = hx - kx;  // column of this pixel in the copy shifted by kx
                if (tx >= 0 && tx < 16) {
                    T* dst = xT + (kx * 32 + wave * 8) * XPP + hy * 16 + tx;
#pragma unroll
                    for (int i = 0; i < 8; ++i) Elem<T>::st(dst + i * XPP, v[i]);
                }
            }
        }
        __syncthreads();
        // ---- MFMA: 4 K-chunks of 32 pixels (= 2 tile rows); wave tiles tt = wave + 4j: ti = tt % 8, tj = tt / 8 (tap = tj/2, ci16 = tj%2)
#pragma unroll
        for (int pc = 0; pc < 4; ++pc) {
            const int kg = lane >> 4;
            const int trow = 2 * pc + (kg >> 1), tcol = (kg & 1) * 8;  // tile row / column start of this lane's 8 pixels
            typename Mma<T>::Frag fa[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) fa[a] = load_swz<T>(dzT + (pc >> 1) * 64, DPP, (wave + 4 * a) * 16, pc & 1, lane);
#pragma unroll
            for (int tj = 0; tj < 18; ++tj) {
                const int tap = tj >> 1, ky = tap / 3, kx = tap % 3;
                const T* src = xT + (kx * 32 + (tj & 1) * 16 + (lane & 15)) * XPP + (trow + ky) * 16 + tcol;
                typename Mma<T>::Frag fb;
                if constexpr (Elem<T>::is_bf16) {
                    fb.q = *reinterpret_cast<const uint4*>(src);
                } else {
                    // fp32 fragment: k-step ks holds pixel ks*4 + kg of the 32-pixel chunk (see Mma<float>)
#pragma unroll
                    for (int ks = 0; ks < 8; ++ks) {
                        const int pk = ks * 4 + kg;  // pixel within the chunk
                        fb.v[ks] = xT[(kx * 32 + (tj & 1) * 16 + (lane & 15)) * XPP + (2 * pc + (pk >> 4) + ky) * 16 + (pk & 15)];
                    }
                }
#pragma unroll
                for (int a = 0; a < 2; ++a) acc[tj * 2 + a] = Mma<T>::template mma<8>(fa[a], fb, acc[tj * 2 + a]);
            }
        }
    }
    // ---- flush: acc[tj*2 + a]: rows co = (wave + 4a)*16 + (lane>>4)*4 + r, column ci = ci_base + (tj&1)*16 + (lane&15), tap = tj>>1
    if (ws) {
        // two-stage, atomic-free and deterministic: this block's partial goes to ws[blockIdx.x][tap][ci][co] with 16-byte stores
        // (4 consecutive co per lane); k_wgrad3x3_reduce sums over blockIdx.x.  (37k float atomics per block were the bottleneck.)
        float* wb = ws + (long)blockIdx.x * 9 * Cin * Cout;
#pragma unroll
        for (int tj = 0; tj < 18; ++tj)
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const int ci = ci_base + (tj & 1) * 16 + (lane & 15), tap = tj >> 1;
                const int co0 = (wave + 4 * a) * 16 + (lane >> 4) * 4;
                if (co0 < Cout) {
                    const f32x4 v = acc[tj * 2 + a];
                    *reinterpret_cast<float4*>(wb + ((long)tap * Cin + ci) * Cout + co0) = make_float4(v[0], v[1], v[2], v[3]);
                }
            }
        return;
    }
#pragma unroll
    for (int tj = 0; tj < 18; ++tj)
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const int ci = ci_base + (tj & 1) * 16 + (lane & 15), tap = tj >> 1;
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
                const int co = (wave + 4 * a) * 16 + (lane >> 4) * 4 + r4;
                if (co < Cout && ci < Cin) atomicAdd(&dW[((long)co * Cin + ci) * 9 + tap], acc[tj * 2 + a][r4]);
            }
        }
}

// bf16 variant on the LDS transpose read (see lds_tr8 in common.h): both tiles are staged in their NATURAL NHWC order with plain 16-byte
// stores (dz tile [128 px][Cout], input halo [10 x 18 px][32 ci]) and the K = pixel operands are produced by ds_read_b64_tr_b16 --
// no transposing ds_write_b16 scatters, no shifted copies -- and the next tile's loads are register-prefetched under the 144 MFMAs.
// Same decomposition and accumulator layout as k_conv3x3_wgrad (so the flush is shared).
template <int COUT_MAX>
__global__ __launch_bounds__(256) void k_conv3x3_wgrad_tr(const bf16* __restrict__ dz, int Cout, const bf16* __restrict__ x, int Cin,
                                                          float* __restrict__ dW, int N, int H, int W, float* __restrict__ ws) {
    constexpr int TH = 8, TW = 16;
    constexpr int DP = COUT_MAX + 8;   // dz tile pitch (elements)
    constexpr int XP = 40;             // halo pitch: 32 ci + 8
    constexpr int NDI = 128 * (COUT_MAX / 8) / 256, NXI = 3;  // 16-byte staging items per thread (dz; x halo: 180 px * 4 groups = 720)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16* dzs = reinterpret_cast<bf16*>(smem);   // [128][DP]
    bf16* xh = dzs + 128 * DP;                   // [180][XP]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ci_base = blockIdx.y * 32;
    const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
    const int ntiles = N * tiles_x * tiles_y;
    const int CG8 = Cout / 8;  // 8-channel groups of dz actually present (<= COUT_MAX / 8)
    f32x4 acc[36];
#pragma unroll
    for (int j = 0; j < 36; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // zero the tiles once: channel columns >= Cout of the dz tile stay zero
    for (int i = tid * 8; i < 128 * DP + 180 * XP; i += 256 * 8) *reinterpret_cast<uint4*>(dzs + i) = make_uint4(0, 0, 0, 0);
    Raw8<bf16> dr[NDI], xr[NXI];
    unsigned okd = 0, okx = 0;
    auto issue = [&](long t) {
        const int tpi = tiles_x * tiles_y;
        const int n = (int)t / tpi, r = (int)t - n * tpi;
        const int h0 = (r / tiles_x) * TH, w0 = (r % tiles_x) * TW;
        okd = okx = 0;
#pragma unroll
        for (int j = 0; j < NDI; ++j) {
            const int it = tid + j * 256, px = it / (COUT_MAX / 8), g8 = it % (COUT_MAX / 8);
            const int h = h0 + px / TW, w = w0 + px % TW;
            const bool ok = h < H && w < W && g8 < CG8;
            dr[j] = load8_raw(ok ? dz + (((long)n * H + h) * W + w) * Cout + g8 * 8 : dz);
            okd |= ok ? 1u << j : 0u;
        }
#pragma unroll
        for (int j = 0; j < NXI; ++j) {
            const int it = tid + j * 256, hp = it >> 2, g8 = it & 3;
            const int h = h0 + hp / 18 - 1, w = w0 + hp % 18 - 1;
            const bool ok = it < 720 && (unsigned)h < (unsigned)H && (unsigned)w < (unsigned)W;
            xr[j] = load8_raw(ok ? x + (((long)n * H + h) * W + w) * Cin + ci_base + g8 * 8 : x);
            okx |= ok ? 1u << j : 0u;
        }
    };
    // tile-invariant operand addresses
    const int i16 = lane & 15, kg = lane >> 4;
    const int prow = 4 * kg + (i16 >> 2), pcol = (i16 & 3) * 4;
    TileSched ts(ntiles);
    if (ts.first < ts.end) issue(ts.first);
    __syncthreads();
    for (long t = ts.first; t < ts.end; t += ts.step) {
#pragma unroll
        for (int j = 0; j < NDI; ++j) {
            const int it = tid + j * 256, px = it / (COUT_MAX / 8), g8 = it % (COUT_MAX / 8);
            *reinterpret_cast<uint4*>(dzs + px * DP + g8 * 8) = (okd & (1u << j)) ? dr[j].a : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < NXI; ++j) {
            const int it = tid + j * 256;
            if (it < 720) *reinterpret_cast<uint4*>(xh + (it >> 2) * XP + (it & 3) * 8) = (okx & (1u << j)) ? xr[j].a : make_uint4(0, 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (t + ts.step < ts.end) issue(t + ts.step);
        lds_barrier();
#pragma unroll
        for (int pc = 0; pc < 4; ++pc) {
            const int p = pc * 32 + prow, ty = p >> 4, tx = p & 15;  // this lane's supplied position (second read: next tile row)
            bf16x8 fa[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const bf16* ap = dzs + p * DP + (wave + 4 * a) * 16 + pcol;
                fa[a] = lds_tr8(ap, ap + 16 * DP);
            }
#pragma unroll
            for (int tj = 0; tj < 18; ++tj) {
                const int tap = tj >> 1, ky = tap / 3, kx = tap % 3;
                const bf16* bp = xh + ((ty + ky) * 18 + tx + kx) * XP + (tj & 1) * 16 + pcol;
                const bf16x8 fb = lds_tr8(bp, bp + 18 * XP);
#pragma unroll
                for (int a = 0; a < 2; ++a) acc[tj * 2 + a] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[a], fb, acc[tj * 2 + a], 0, 0, 0);
            }
        }
        lds_barrier();
    }
    // ---- flush (same accumulator layout as k_conv3x3_wgrad)
    if (ws) {
        float* wb = ws + (long)blockIdx.x * 9 * Cin * Cout;
#pragma unroll
        for (int tj = 0; tj < 18; ++tj)
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const int ci = ci_base + (tj & 1) * 16 + (lane & 15), tap = tj >> 1;
                const int co0 = (wave + 4 * a) * 16 + (lane >> 4) * 4;
                if (co0 < Cout) {
                    const f32x4 v = acc[tj * 2 + a];
                    *reinterpret_cast<float4*>(wb + ((long)tap * Cin + ci) * Cout + co0) = make_float4(v[0], v[1], v[2], v[3]);
                }
            }
        return;
    }
#pragma unroll
    for (int tj = 0; tj < 18; ++tj)
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const int ci = ci_base + (tj & 1) * 16 + (lane & 15), tap = tj >> 1;
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
                const int co = (wave + 4 * a) * 16 + (lane >> 4) * 4 + r4;
                if (co < Cout && ci < Cin) atomicAdd(&dW[((long)co * Cin + ci) * 9 + tap], acc[tj * 2 + a][r4]);
            }
        }
}

// ---------------------------------------------------------------------------------------------------------------------
// The gathered weight gradient in the natural-layout + LDS-transpose-read form of k_wgrad_gemm_x3 (bf16, workspace flush):
//   D[ra][jc] = sum_pos A~[pos][ra] * B[pos * stride + tap(jc) - pad][cb(jc)],   jc = tap * CB + cb.
// k_wgrad_gather<bf16> builds TRANSPOSED [channel][position] tiles with two-byte scatter stores and holds 16 accumulator tiles + two tiles of
// prefetch per thread (256 VGPRs + 127 AGPRs: one block owns a CU, ~50 TFLOP/s -- and on the detection step's side stream such a block keeps a CU
// from the main stream's kernels for 100 us).  Here a chunk of 32 positions is staged as it lies in memory ([position][channel], 16-byte
// vectors; gathered rows outside B are zero) and both MFMA operands come from ds_read_b64_tr_b16; block = 128 x 128 outputs over a contiguous
// range of chunks, next chunk register-prefetched, partial -> the workspace layout of k_wgrad_gather_reduce.
__global__ __launch_bounds__(256, 2) void k_wgrad_gather_tr(const bf16* __restrict__ A, int ldA, int CA, const float* __restrict__ trA, const bf16* __restrict__ B,
                                                            int ldB, int CB, int N, int hA, int wA, int HB, int WB, int stride, int padh, int padw, int KW,
                                                            int ntaps, float* __restrict__ ws, int tiles_a, int chunks_per_block) {
    constexpr int BM = 128, KC = 32, PA = BM + 8;
    __shared__ __attribute__((aligned(16))) bf16 At[KC * PA];
    __shared__ __attribute__((aligned(16))) bf16 Bt[KC * PA];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ta = blockIdx.y % tiles_a, tj = blockIdx.y / tiles_a;
    const int a0 = ta * BM, j0 = tj * BM;
    const int J = ntaps * CB, CA8 = (CA + 7) & ~7;
    const long P = (long)N * hA * wA;
    const long nchunks = (P + KC - 1) / KC;
    const long c_first = (long)blockIdx.x * chunks_per_block, c_end = c_first + chunks_per_block < nchunks ? c_first + chunks_per_block : nchunks;
    // staging map: item f = tid + 256 j (j < 2): row f >> 4 of the chunk, columns (f & 15) * 8 .. + 7 of the block's 128
    const int col8 = (tid & 15) * 8;
    const bool cola = a0 + col8 < CA8, colb = j0 + col8 < J;
    const int tapb = colb ? (j0 + col8) / CB : 0, cb0 = j0 + col8 - tapb * CB;
    const int dyb = tapb / KW - padh, dxb = tapb % KW - padw;
    float sc[8], sh[8], lo[8];
    if (trA && cola) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int c = a0 + col8 + i < CA ? a0 + col8 + i : 0;
            sc[i] = trA[c];
            sh[i] = trA[CA + c];
            lo[i] = trA[2 * CA + c];
        }
    }
    uint4 ra[2], rb[2];
    unsigned ok = 0;  // bits 0-1: A rows inside P, bits 2-3: B rows inside the gathered tensor
    auto issue = [&](long c) {
        ok = 0;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const long p = c * KC + (tid >> 4) + 16 * j;
            const bool inp = p < P;
            const PixIdx q = decode_pixel(inp ? p : 0, hA, wA);
            const bool oka = inp && cola;
            ra[j] = *reinterpret_cast<const uint4*>(oka ? A + p * ldA + a0 + col8 : A);
            const int Y = q.h * stride + dyb, X = q.w * stride + dxb;
            const bool okb = inp && colb && (unsigned)Y < (unsigned)HB && (unsigned)X < (unsigned)WB;
            rb[j] = *reinterpret_cast<const uint4*>(okb ? B + (((long)q.n * HB + Y) * WB + X) * ldB + cb0 : B);
            ok |= (oka ? 1u : 0u) << j | (okb ? 4u : 0u) << j;
        }
    };
    const int wm = wave & 1, wn = wave >> 1;  // 2 x 2 waves, each 4 x 4 MFMA tiles of 16 x 16
    const int prow = 4 * (lane >> 4) + ((lane & 15) >> 2), pcol = (lane & 3) * 4;
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (c_first < c_end) issue(c_first);
    for (long c = c_first; c < c_end; ++c) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int off = ((tid >> 4) + 16 * j) * PA + col8;
            uint4 va = make_uint4(0, 0, 0, 0);
            if (ok & (1u << j)) {
                va = ra[j];
                if (trA) {
                    float v[8];
                    unpack8(Raw8<bf16>{va}, v);
#pragma unroll
                    for (int i = 0; i < 8; ++i) v[i] = fmaxf(fmaf(v[i], sc[i], sh[i]), lo[i]);
                    va = make_uint4(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7]));
                }
            }
            *reinterpret_cast<uint4*>(At + off) = va;
            *reinterpret_cast<uint4*>(Bt + off) = (ok & (4u << j)) ? rb[j] : make_uint4(0, 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (c + 1 < c_end) issue(c + 1);
        lds_barrier();
        bf16x8 af[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int o = prow * PA + (wm * 4 + i) * 16 + pcol;
            af[i] = lds_tr8(At + o, At + o + 16 * PA);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int o = prow * PA + (wn * 4 + j) * 16 + pcol;
            const bf16x8 bfr = lds_tr8(Bt + o, Bt + o + 16 * PA);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr, acc[i][j], 0, 0, 0);
        }
        lds_barrier();
    }
    // partial -> ws[blockIdx.x][jc][ra] (CA8-padded rows), 4 consecutive ra per lane
    float* wb = ws + (long)blockIdx.x * J * CA8;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r0 = a0 + (wm * 4 + i) * 16 + (lane >> 4) * 4, jc = j0 + (wn * 4 + j) * 16 + (lane & 15);
            if (r0 < CA8 && jc < J) {
                const f32x4 v = acc[i][j];
                *reinterpret_cast<float4*>(wb + (long)jc * CA8 + r0) = make_float4(v[0], v[1], v[2], v[3]);
            }
        }
}

static void wgrad_gather_tr_grid(int CA, int CB, int ntaps, long P, int& gx, int& gy, int& tiles_a, int& cpb) {
    tiles_a = (((CA + 7) & ~7) + 127) / 128;
    gy = tiles_a * ((ntaps * CB + 127) / 128);
    const long nchunks = (P + 31) / 32;
    constexpr int target = 1024;  // K splits: >= 8 chunks per block, ~4 blocks per CU in total
    long g = target / gy;
    if (g > nchunks / 8) g = nchunks / 8;
    // every K split writes (and the reducer re-reads) a full ntaps * CB * CA8 partial: keep the workspace around 16 MB
    const long part_bytes = (long)ntaps * CB * ((CA + 7) & ~7) * 4, by_ws = (16L << 20) / part_bytes;
    if (g > by_ws) g = by_ws < 8 ? 8 : by_ws;
    if (g < 1) g = 1;
    cpb = (int)((nchunks + g - 1) / g);
    gx = (int)((nchunks + cpb - 1) / cpb);
}
static void wgrad_gather_grid(int CA, int CB, int ntaps, long P, int dtype, long& gx, int& gy) {
    if (dtype == 1) {  // bf16: k_wgrad_gather_tr
        int g, ta, cpb;
        wgrad_gather_tr_grid(CA, CB, ntaps, P, g, gy, ta, cpb);
        gx = g;
        return;
    }
    const long ntiles = (P + 63) / 64;  // fp32: k_wgrad_gather<float, 64>
    const int CA8 = (CA + 7) & ~7;
    gy = ((CA8 + 127) / 128) * ((ntaps * CB + 127) / 128);
    constexpr int target = 512;  // two 4-wave blocks per CU (round 4: one wave per SIMD cannot keep the MFMA pipe busy -- tools/probes/mfma_issue_probe.hip; 256 -> 512: 0.563 -> 0.496 ms per step, 768: 0.59)  // few flushing blocks, each loops over many tiles
    gx = ntiles / 4;
    if (gx < 1) gx = 1;
    long cap = target / gy;
    if (cap < 8) cap = 8;
    if (gx > cap) gx = cap;
    if (gx >= 8) gx &= ~7L;
}

// ---------------------------------------------------------------------------------------------------------------------
// Split-bf16 ("bf16x3") weight-gradient GEMM for fp32 operands:  dW[ra][cb] += sum_p A[p][ra] * B[p][cb]   (K = P rows).
// The GRU / Linear weight gradients of the CRNN are fp32 (the reference keeps the GRU in fp32 under autocast, models.py:264-266) and
// were the largest item of the CRNN step on the exact-fp32 MFMA (v_mfma_f32_16x16x4_f32 is 1/16 of the bf16 rate).  In THROUGHPUT mode
// they run here as  a*b ~ ah*bh + ah*bl + al*bh  with  ah = bf16(a), al = bf16(a - ah)  (dropped term and residuals <= ~1.1e-5 relative
// per product, fp32 accumulation: the same order as the summation-order noise of an fp32 dot product of K = 25856 terms); parity
// (fp32) mode keeps the exact-fp32 kernel.  Operands are staged in natural [row][channel] order as hi / lo bf16 planes and read with
// the LDS transpose read (K = rows).  Block = 128 x 128 outputs, a contiguous range of 32-row chunks; partials -> workspace in the
// layout of k_wgrad_gather_reduce (ntaps = 1).
__global__ __launch_bounds__(256) void k_wgrad_gemm_x3(const float* __restrict__ A, int ldA, int CA, const float* __restrict__ B, int ldB, int CB, long P,
                                                       float* __restrict__ ws, int tiles_a, int chunks_per_block) {
    constexpr int BM = 128, BN = 128, KC = 32, PA = BM + 8;  // pitch (elements) of the bf16 planes
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16* Ah = reinterpret_cast<bf16*>(smem);  // [KC][PA]
    bf16* Al = Ah + KC * PA;
    bf16* Bh = Al + KC * PA;
    bf16* Bl = Bh + KC * PA;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ta = blockIdx.y % tiles_a, tb = blockIdx.y / tiles_a;
    const int a0 = ta * BM, b0 = tb * BN;
    const long nchunks = (P + KC - 1) / KC;
    const long c_first = (long)blockIdx.x * chunks_per_block, c_end = c_first + chunks_per_block < nchunks ? c_first + chunks_per_block : nchunks;
    // staging map: 4 float4 of A and 4 of B per thread and chunk: f = tid + 256*j -> row f/32, columns (f%32)*4..+3
    float4 ra[4], rb[4];
    auto issue = [&](long c) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int f = tid + j * 256, row = f >> 5, col = (f & 31) * 4;
            const long p = c * KC + row;
            const bool oka = p < P && a0 + col < CA, okb = p < P && b0 + col < CB;  // CB a multiple of 4, A rows padded to one (checked by the host)
            ra[j] = oka ? *reinterpret_cast<const float4*>(A + p * ldA + a0 + col) : make_float4(0.f, 0.f, 0.f, 0.f);
            rb[j] = okb ? *reinterpret_cast<const float4*>(B + p * ldB + b0 + col) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto split_store = [&](const float4& v, bf16* hi, bf16* lo, int off) {
        const float x[4] = {v.x, v.y, v.z, v.w};
        float h[4], l[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            h[i] = Elem<bf16>::round(x[i]);
            l[i] = x[i] - h[i];
        }
        *reinterpret_cast<uint2*>(hi + off) = make_uint2(pack2bf(h[0], h[1]), pack2bf(h[2], h[3]));
        *reinterpret_cast<uint2*>(lo + off) = make_uint2(pack2bf(l[0], l[1]), pack2bf(l[2], l[3]));
    };
    const int wm = wave & 1, wn = wave >> 1;  // 2 x 2 waves, each 4 x 4 MFMA tiles of 16 x 16
    const int prow = 4 * (lane >> 4) + ((lane & 15) >> 2), pcol = (lane & 3) * 4;
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (c_first < c_end) issue(c_first);
    for (long c = c_first; c < c_end; ++c) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int f = tid + j * 256, off = (f >> 5) * PA + (f & 31) * 4;
            split_store(ra[j], Ah, Al, off);
            split_store(rb[j], Bh, Bl, off);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (c + 1 < c_end) issue(c + 1);
        lds_barrier();
        bf16x8 ah[4], al[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int o = prow * PA + (wm * 4 + i) * 16 + pcol;
            ah[i] = lds_tr8(Ah + o, Ah + o + 16 * PA);
            al[i] = lds_tr8(Al + o, Al + o + 16 * PA);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int o = prow * PA + (wn * 4 + j) * 16 + pcol;
            const bf16x8 bh = lds_tr8(Bh + o, Bh + o + 16 * PA), bl = lds_tr8(Bl + o, Bl + o + 16 * PA);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bh, acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bl, acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[i], bh, acc[i][j], 0, 0, 0);
            }
        }
        lds_barrier();
    }
    // partial -> ws[blockIdx.x][cb][ra] (CA8-padded rows), 4 consecutive ra per lane
    const int CA8 = (CA + 7) & ~7;
    float* wb = ws + (long)blockIdx.x * CB * CA8;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r0 = a0 + (wm * 4 + i) * 16 + (lane >> 4) * 4, cb = b0 + (wn * 4 + j) * 16 + (lane & 15);
            if (r0 < CA8 && cb < CB) {
                const f32x4 v = acc[i][j];
                *reinterpret_cast<float4*>(wb + (long)cb * CA8 + r0) = make_float4(v[0], v[1], v[2], v[3]);
            }
        }
}
static void wgrad_x3_grid(int CA, int CB, long P, int& gx, int& gy, int& tiles_a, int& cpb) {
    tiles_a = (CA + 127) / 128;
    gy = tiles_a * ((CB + 127) / 128);
    const long nchunks = (P + 31) / 32;
    constexpr int target = 512;  // (two resident 4-wave workgroups per CU; 384 / 768 / 1024 measured: no better)
    long g = target / gy;
    if (g < 1) g = 1;
    if (g > nchunks) g = nchunks;
    cpb = (int)((nchunks + g - 1) / g);
    gx = (int)((nchunks + cpb - 1) / cpb);
}

static int wgrad3x3_gx(int Cin, int N, int H, int W) {
    const int ntiles = N * ((W + 15) / 16) * ((H + 7) / 8);
    const int gy = Cin / 32;
    constexpr int target = 512;  // two 4-wave blocks per CU (see wgrad_gather_grid)
    long gx = ntiles / 4;
    if (gx < 1) gx = 1;
    long cap = target / gy;
    if (cap < 8) cap = 8;
    if (gx > cap) gx = cap;
    if (gx >= 8) gx &= ~7L;
    return (int)gx;
}

__global__ __launch_bounds__(256) void k_wgrad3x3_reduce(const float* __restrict__ ws, int gx, int Cout, int Cin, float* __restrict__ dW) {
    const long n = 9L * Cin * Cout;  // grid ceil(n / 32): see k_wgrad_gather_reduce
    const long i = (long)blockIdx.x * 32 + (threadIdx.x & 31);
    float s;
    if (!det_column_sum(ws, gx, n, i, s)) return;
    const int co = (int)(i % Cout), ci = (int)((i / Cout) % Cin), tap = (int)(i / ((long)Cout * Cin));
    dW[((long)co * Cin + ci) * 9 + tap] += s;
}

extern "C" {

// workspace (floats) for the atomic-free flush of ocrs_wgrad_gather
long ocrs_wgrad_gather_ws_floats(int CA, int CB, int ntaps, long P, int dtype) {
    long gx;
    int gy;
    wgrad_gather_grid(CA, CB, ntaps, P, dtype, gx, gy);
    return gx * ntaps * CB * ((CA + 7) & ~7);
}

// Weight gradient by gathering: dW[(ra*CB + cb)*KH*KW + tap] += sum_pos A~[pos][ra] * B[pos*stride + tap - pad][cb].
//   Conv2d: A = dz [N][Ho][Wo][Cout], B = x; Linear / GRU: KH=KW=1, hA=1.  trA (nullable) = load transform of A.
//   ws: workspace of ocrs_wgrad_gather_ws_floats() floats (deterministic two-stage reduction) or null (float atomics into dW).
int ocrs_wgrad_gather(const void* A, int ldA, int CA, const float* trA, const void* B, int ldB, int CB, float* dW, float* ws, int N, int hA,
                      int wA, int HB, int WB, int stride, int padh, int padw, int KH, int KW, int dtype, hipStream_t st) {
    OCRS_CHECK_ARG(A && B && dW && CB % 8 == 0 && ldA % 8 == 0 && ldB % 8 == 0 && ldA >= ((CA + 7) & ~7) && ldB >= CB);
    const long P = (long)N * hA * wA;
    OCRS_CHECK_ARG(P < (1L << 31));
    long gx;
    int gy;
    wgrad_gather_grid(CA, CB, KH * KW, P, dtype, gx, gy);
    if (int rc = dtype == 1 ? dyn_lds<&k_wgrad_gather<bf16, 128>>(96 * 1024) : dyn_lds<&k_wgrad_gather<float, 64>>(96 * 1024)) return rc;
    if (dtype == 1 && ws) {
        int g, gy2, ta, cpb;
        wgrad_gather_tr_grid(CA, CB, KH * KW, P, g, gy2, ta, cpb);
        hipLaunchKernelGGL(k_wgrad_gather_tr, dim3(g, gy2), dim3(256), 0, st, (const bf16*)A, ldA, CA, trA, (const bf16*)B, ldB, CB, N, hA, wA, HB, WB, stride,
                           padh, padw, KW, KH * KW, ws, ta, cpb);
    } else if (dtype == 1)
        hipLaunchKernelGGL((k_wgrad_gather<bf16, 128>), dim3((int)gx, gy), dim3(256), 2 * 128 * 136 * 2, st, (const bf16*)A, ldA, CA, trA, (const bf16*)B,
                           ldB, CB, dW, N, hA, wA, HB, WB, stride, padh, padw, KH, KW, ws);
    else
        hipLaunchKernelGGL((k_wgrad_gather<float, 64>), dim3((int)gx, gy), dim3(256), 2 * 128 * 68 * 4, st, (const float*)A, ldA, CA, trA,
                           (const float*)B, ldB, CB, dW, N, hA, wA, HB, WB, stride, padh, padw, KH, KW, ws);
    if (ws) {
        const int CA8 = (CA + 7) & ~7;
        const long n = (long)KH * KW * CB * CA8;
        hipLaunchKernelGGL(k_wgrad_gather_reduce, dim3((int)((n + 31) / 32)), dim3(256), 0, st, ws, (int)gx, CA, CA8, CB,
                           KH * KW, dW);
    }
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

// Split-bf16 weight-gradient GEMM for fp32 operands (throughput mode of the GRU / Linear weight gradients):
//   dW [CA][CB] += A^T B,  A [P][ldA] (first CA columns), B [P][ldB] (first CB columns), CA, CB, ldA, ldB multiples of 4.
//   ws: ocrs_wgrad_gemm_x3_ws_floats() floats.  Products carry <= ~1.1e-5 relative error (see k_wgrad_gemm_x3), fp32 accumulation.
long ocrs_wgrad_gemm_x3_ws_floats(int CA, int CB, long P) {
    int gx, gy, ta, cpb;
    wgrad_x3_grid(CA, CB, P, gx, gy, ta, cpb);
    return (long)gx * CB * ((CA + 7) & ~7);
}
int ocrs_wgrad_gemm_x3(const float* A, int ldA, int CA, const float* B, int ldB, int CB, float* dW, float* ws, long P, hipStream_t st) {
    // (a ragged CA -- the class count of the output Linear -- is fine as long as the rows of A extend to the next multiple of 4: the extra
    // columns are loaded, their partials land in the CA8-padded workspace rows and the reduce skips them)
    OCRS_CHECK_ARG(A && B && dW && ws && P > 0 && CB % 4 == 0 && ldA % 4 == 0 && ldB % 4 == 0 && ldA >= ((CA + 3) & ~3) && ldB >= CB);
    OCRS_CHECK_ARG((reinterpret_cast<uintptr_t>(A) & 15) == 0 && (reinterpret_cast<uintptr_t>(B) & 15) == 0);
    int gx, gy, ta, cpb;
    wgrad_x3_grid(CA, CB, P, gx, gy, ta, cpb);
    hipLaunchKernelGGL(k_wgrad_gemm_x3, dim3(gx, gy), dim3(256), 4 * 32 * 136 * 2, st, A, ldA, CA, B, ldB, CB, P, ws, ta, cpb);
    const int CA8 = (CA + 7) & ~7;
    const long n = (long)CB * CA8;
    hipLaunchKernelGGL(k_wgrad_gather_reduce, dim3((int)((n + 31) / 32)), dim3(256), 0, st, ws, gx, CA, CA8, CB, 1, dW);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

// workspace (floats) for the atomic-free flush of ocrs_conv3x3_wgrad
long ocrs_conv3x3_wgrad_ws_floats(int Cout, int Cin, int N, int H, int W) { return (long)wgrad3x3_gx(Cin, N, H, W) * 9 * Cin * Cout; }

// Conv2d 3x3 / stride 1 / pad 1 weight gradient (Cout <= 128, Cin % 32 == 0): dW [Cout][Cin][3][3] += ...
// ws: workspace of ocrs_conv3x3_wgrad_ws_floats() floats (deterministic two-stage reduction), or null (float atomics).
int ocrs_conv3x3_wgrad(const void* dz, int Cout, const void* x, int Cin, float* dW, float* ws, int N, int H, int W, int dtype, hipStream_t st) {
    OCRS_CHECK_ARG(dz && x && dW && Cout % 8 == 0 && Cout <= 128 && Cin % 32 == 0);
    const int gy = Cin / 32;
    const long gx = wgrad3x3_gx(Cin, N, H, W);  // few flushing blocks: each loops over many tiles
    if (int rc = dtype != 1    ? dyn_lds<&k_conv3x3_wgrad<float>>(140 * 1024)
                 : Cout > 64 ? dyn_lds<&k_conv3x3_wgrad_tr<128>>(64 * 1024)
                             : dyn_lds<&k_conv3x3_wgrad_tr<64>>(64 * 1024))
        return rc;
    if (dtype == 1) {
        if (Cout > 64)
            hipLaunchKernelGGL(k_conv3x3_wgrad_tr<128>, dim3((int)gx, gy), dim3(256), (128 * 136 + 180 * 40) * 2, st, (const bf16*)dz, Cout, (const bf16*)x,
                               Cin, dW, N, H, W, ws);
        else
            hipLaunchKernelGGL(k_conv3x3_wgrad_tr<64>, dim3((int)gx, gy), dim3(256), (128 * 72 + 180 * 40) * 2, st, (const bf16*)dz, Cout, (const bf16*)x,
                               Cin, dW, N, H, W, ws);
    } else
        hipLaunchKernelGGL(k_conv3x3_wgrad<float>, dim3((int)gx, gy), dim3(256), (128 * 132 + 96 * 164) * 4, st, (const float*)dz, Cout,
                           (const float*)x, Cin, dW, N, H, W, ws);
    if (ws) hipLaunchKernelGGL(k_wgrad3x3_reduce, dim3((9 * Cin * Cout + 31) / 32), dim3(256), 0, st, ws, (int)gx, Cout, Cin, dW);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

}  // extern "C"
