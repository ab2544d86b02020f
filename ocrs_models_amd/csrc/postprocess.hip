// Word-level validation metrics of the detection test() loop on the device (ocrs_models/postprocess.py:11-36 extract_cc_quads,
// :102-187 box_match_metrics; train_detection.py:177-184), restating the host numpy contract of ocrs_models_amd/postprocess.py.
//
//   labelling (per side)  k_cc_local    binarise + 8-connected union-find of a 64x16 tile in LDS (root = minimum raster index)
//                         k_cc_border   merges across tile borders: global union-find with atomicMin (the smaller index wins)
//                         k_cc_flatten  path compression; roots counted per 1024-pixel chunk
//                         k_scan_chunks per-image exclusive scan -> component count and the chunk offsets
//                         k_cc_number   component id = rank of the root in raster order (scipy.ndimage.label's numbering)
//                         k_cc_labels   (optional) the label image
//   quads (per side)      k_cc_ymax     last row of each component (run left ends only)
//                         k_cc_rowoff   per-image scan of component heights -> slots of the per-row extents
//                         k_cc_rows     per component and row: min / max x (run ends only: the only pixels that can be hull vertices)
//                         k_cc_quad     one thread per component: monotone-chain hull of the row extremes, rotating calipers in fp64
//   box match             k_bm_count    targets bucketed by floor(bbox x-min); per-image widest target
//                         k_bm_scan     bucket offsets;   k_bm_scatter   target ids sorted by bucket
//                         k_bm_pairs    one thread per prediction, over the targets whose bbox can overlap it: strict bbox prefilter,
//                                       Sutherland-Hodgman in fp64, IoU / coverage counts (integer atomics)
//                         k_bm_final    the four numbers per image (fp64)
//
// Every count the launches need is read on the device: grids are sized from (B, H, W) and kernels leave early.  No host sync, no
// allocation; the caller provides the workspace (sizes: ocrs_*_ws_bytes).
//
// The geometry follows the host's arithmetic operation by operation, so FMA contraction is off in this file; where the host itself fuses
// (numpy's dot / 2-term matmul go through BLAS, whose kernels use fma) the same fma is written out, and np.hypot is glibc's correction
// kernel.  Integer work (labelling, hull construction) is exact.
#include "common.h"
#include "quad_geom.h"  // host_dot_rolled, shoelace2, area_of, quad_inter, load_quad (shared with ocr_eval.hip)

#pragma clang fp contract(off)

namespace {

constexpr int TW = 64, TH = 16, TPX = TW * TH;  // labelling tile: 64 columns x 16 rows, 256 threads x 4 pixels
constexpr int CHUNK = 1024;                        // pixels per block of the flatten / number / run-end passes

__host__ __device__ inline long cdiv(long a, long b) { return (a + b - 1) / b; }

// ------------------------------------------------------------------ union-find (root = smallest index of the set) ----------
template <int SCOPE>
__device__ __forceinline__ int ld_relaxed(int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, SCOPE); }

template <int SCOPE>
__device__ __forceinline__ int uf_find(int* L, int x) {
    for (;;) {
        const int p = ld_relaxed<SCOPE>(L + x);
        if (p == x) return x;
        x = p;
    }
}

// L[x] <= x always and only ever decreases, so every chain ends at the smallest index of its set.
template <int SCOPE>
__device__ void uf_merge(int* L, int a, int b) {
    for (;;) {
        a = uf_find<SCOPE>(L, a);
        b = uf_find<SCOPE>(L, b);
        if (a == b) return;
        if (a < b) {
            const int old = __hip_atomic_fetch_min(L + b, a, __ATOMIC_RELAXED, SCOPE);
            if (old == b) return;
            b = old;
        } else {
            const int old = __hip_atomic_fetch_min(L + a, b, __ATOMIC_RELAXED, SCOPE);
            if (old == a) return;
            a = old;
        }
    }
}

// exclusive prefix of a 0/1 flag over a 256-thread block in thread order; total returned through *tot
__device__ __forceinline__ int block_rank256(bool f, int* s_w, int* tot) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long m = __ballot(f);
    const int below = __popcll(m & ((1ull << lane) - 1ull));
    __syncthreads();
    if (lane == 0) s_w[w] = __popcll(m);
    __syncthreads();
    int off = 0;
    for (int i = 0; i < w; ++i) off += s_w[i];
    *tot = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    return off + below;
}

// in-place exclusive scan of v[0..n) (int) by one 1024-thread block; returns the total (identical in every thread)
__device__ long block_scan_excl(int* v, long n, int* s_w) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    long carry = 0;
    for (long base = 0; base < n; base += 1024) {
        const long i = base + threadIdx.x;
        const int x = i < n ? v[i] : 0;
        int inc = x;
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(inc, d);
            if (lane >= d) inc += t;
        }
        __syncthreads();
        if (lane == 63) s_w[w] = inc;
        __syncthreads();
        int woff = 0, all = 0;
        for (int k = 0; k < 16; ++k) {
            woff += k < w ? s_w[k] : 0;
            all += s_w[k];
        }
        if (i < n) v[i] = (int)(carry + woff + inc - x);
        carry += all;
    }
    return carry;
}

// ------------------------------------------------------------------ labelling ----------------------------------------------
template <int KIND>
__global__ __launch_bounds__(256) void k_cc_local(const void* __restrict__ mask, float thr, int* __restrict__ L, int H, int W, long LH,
                                                  int tilesX) {
    __shared__ int s[TPX];
    const int b = blockIdx.y;
    const int tx0 = (blockIdx.x % tilesX) * TW, ty0 = (blockIdx.x / tilesX) * TH;
    const size_t img = (size_t)b * H * W;
    int* Lb = L + (size_t)b * LH;
    const int lx = threadIdx.x & 63;
    bool fg[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ly = (threadIdx.x >> 6) + 4 * k, x = tx0 + lx, y = ty0 + ly;
        bool f = false;
        if (x < W && y < H) {
            const size_t i = img + (size_t)y * W + x;
            f = KIND == 0 ? (static_cast<const float*>(mask)[i] > thr) : (static_cast<const uint8_t*>(mask)[i] != 0);
        }
        fg[k] = f;
        s[ly * TW + lx] = f ? ly * TW + lx : -1;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!fg[k]) continue;
        const int ly = (threadIdx.x >> 6) + 4 * k, l = ly * TW + lx;
        // the neighbours that precede the pixel in raster order: left, up-left, up, up-right (inside the tile)
        if (lx > 0 && s[l - 1] >= 0) uf_merge<__HIP_MEMORY_SCOPE_WORKGROUP>(s, l, l - 1);
        if (ly > 0) {
            if (lx > 0 && s[l - TW - 1] >= 0) uf_merge<__HIP_MEMORY_SCOPE_WORKGROUP>(s, l, l - TW - 1);
            if (s[l - TW] >= 0) uf_merge<__HIP_MEMORY_SCOPE_WORKGROUP>(s, l, l - TW);
            if (lx < TW - 1 && s[l - TW + 1] >= 0) uf_merge<__HIP_MEMORY_SCOPE_WORKGROUP>(s, l, l - TW + 1);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int ly = (threadIdx.x >> 6) + 4 * k, x = tx0 + lx, y = ty0 + ly;
        if (x >= W || y >= H) continue;
        int v = -1;
        if (fg[k]) {
            const int r = uf_find<__HIP_MEMORY_SCOPE_WORKGROUP>(s, ly * TW + lx);
            v = (ty0 + r / TW) * W + tx0 + r % TW;  // the tile's raster order is the image's: the local root is the smallest global index
        }
        Lb[(size_t)y * W + x] = v;
    }
}

// one block per tile: the pixels of its first row, first column and last column merge with preceding neighbours in other tiles
__global__ __launch_bounds__(128) void k_cc_border(int* __restrict__ L, int H, int W, long LH, int tilesX) {
    const int b = blockIdx.y, t = threadIdx.x;
    const int tx0 = (blockIdx.x % tilesX) * TW, ty0 = (blockIdx.x / tilesX) * TH;
    int x, y;
    if (t < TW) {
        x = tx0 + t;
        y = ty0;
    } else if (t < TW + TH) {
        x = tx0;
        y = ty0 + t - TW;
    } else if (t < TW + 2 * TH) {
        x = tx0 + TW - 1;
        y = ty0 + t - TW - TH;
    } else {
        return;
    }
    if (x >= W || y >= H) return;
    int* Lb = L + (size_t)b * LH;
    const int p = y * W + x;
    if (Lb[p] < 0) return;
    const int dx[4] = {-1, -1, 0, 1}, dy[4] = {0, -1, -1, -1};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int nx = x + dx[k], ny = y + dy[k];
        if (nx < 0 || nx >= W || ny < 0) continue;
        if (nx / TW == x / TW && ny / TH == y / TH) continue;  // same tile: done by k_cc_local
        const int n = ny * W + nx;
        if (ld_relaxed<__HIP_MEMORY_SCOPE_AGENT>(Lb + n) >= 0) uf_merge<__HIP_MEMORY_SCOPE_AGENT>(Lb, p, n);
    }
}

__global__ __launch_bounds__(256) void k_cc_flatten(int* __restrict__ L, long HW, long LH, int* __restrict__ chunk, int nch) {
    __shared__ int s_w[4];
    const int b = blockIdx.y;
    int* Lb = L + (size_t)b * LH;
    int cnt = 0;
    for (int k = 0; k < CHUNK / 256; ++k) {
        const long p = (long)blockIdx.x * CHUNK + k * 256 + threadIdx.x;
        if (p < HW && Lb[p] >= 0) {
            const int r = uf_find<__HIP_MEMORY_SCOPE_AGENT>(Lb, (int)p);
            Lb[p] = r;
            cnt += r == p;
        }
    }
    for (int d = 32; d > 0; d >>= 1) cnt += __shfl_down(cnt, d);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) chunk[(size_t)b * nch + blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// one 1024-thread block per image: exclusive scan of v[b][0..n) in place; total -> tot[b]
__global__ __launch_bounds__(1024) void k_scan_chunks(int* __restrict__ v, long n, int* __restrict__ tot) {
    __shared__ int s_w[16];
    const long t = block_scan_excl(v + (size_t)blockIdx.x * n, n, s_w);
    if (threadIdx.x == 0) tot[blockIdx.x] = (int)t;
}

// component id of a foreground pixel once k_cc_number has run: a root holds -(id + 2), any other pixel its root's index
__device__ __forceinline__ int cc_id(const int* Lb, long p) {
    const int v = Lb[p];
    return v < -1 ? -v - 2 : -Lb[v] - 2;
}
__device__ __forceinline__ bool id_ok(int id, long C) { return id >= 0 && id < C; }  // always true (at most C components); guards the writes

__global__ __launch_bounds__(256) void k_cc_number(int* __restrict__ L, int W, long HW, long LH, const int* __restrict__ choff, int nch,
                                                   int* __restrict__ cy0, int* __restrict__ cy1, long C) {
    __shared__ int s_w[4];
    const int b = blockIdx.y;
    int* Lb = L + (size_t)b * LH;
    int off = choff[(size_t)b * nch + blockIdx.x];
    for (int k = 0; k < CHUNK / 256; ++k) {
        const long p = (long)blockIdx.x * CHUNK + k * 256 + threadIdx.x;
        const bool root = p < HW && Lb[p] == p;
        int tot;
        const int id = off + block_rank256(root, s_w, &tot);
        if (root && id < C) {
            Lb[p] = -id - 2;
            cy0[(size_t)b * C + id] = (int)(p / W);
            cy1[(size_t)b * C + id] = (int)(p / W);
        }
        off += tot;
    }
}

// optional label image: 0 = background, id + 1 otherwise (scipy.ndimage.label's values)
__global__ __launch_bounds__(256) void k_cc_labels(const int* __restrict__ L, long HW, long LH, int* __restrict__ labels) {
    const int b = blockIdx.y;
    const int* Lb = L + (size_t)b * LH;
    for (int k = 0; k < CHUNK / 256; ++k) {
        const long p = (long)blockIdx.x * CHUNK + k * 256 + threadIdx.x;
        if (p < HW) labels[(size_t)b * HW + p] = Lb[p] == -1 ? 0 : cc_id(Lb, p) + 1;  // (labels is [B][H][W]: no id-indexed write)
    }
}

__global__ __launch_bounds__(256) void k_cc_ymax(const int* __restrict__ L, int W, long HW, long LH, int* __restrict__ cy1, long C) {
    const int b = blockIdx.y;
    const int* Lb = L + (size_t)b * LH;
    for (int k = 0; k < CHUNK / 256; ++k) {
        const long p = (long)blockIdx.x * CHUNK + k * 256 + threadIdx.x;
        if (p >= HW || Lb[p] == -1) continue;
        const int x = (int)(p % W);
        if (x > 0 && Lb[p - 1] != -1) continue;  // not the left end of a run
        const int id = cc_id(Lb, p);
        if (id_ok(id, C)) atomicMax(cy1 + (size_t)b * C + id, (int)(p / W));
    }
}

// one 1024-thread block per image: row slots of every component (exclusive scan of the heights), initialised to (INT_MAX, -1)
__global__ __launch_bounds__(1024) void k_cc_rowoff(const int* __restrict__ ncomp, const int* __restrict__ cy0, const int* __restrict__ cy1,
                                                    int* __restrict__ crow, int* __restrict__ row, long C, long rowcap) {
    __shared__ int s_w[16];
    const int b = blockIdx.x;
    const long n = min((long)ncomp[b], C);
    int* cr = crow + (size_t)b * C;
    for (long i = threadIdx.x; i < n; i += 1024) cr[i] = cy1[(size_t)b * C + i] - cy0[(size_t)b * C + i] + 1;
    __syncthreads();
    block_scan_excl(cr, n, s_w);
    __syncthreads();
    int* rb = row + (size_t)b * rowcap * 2;
    for (long i = threadIdx.x; i < n; i += 1024) {
        const long o = cr[i], h = cy1[(size_t)b * C + i] - cy0[(size_t)b * C + i] + 1;
        for (long r = o; r < o + h && r < rowcap; ++r) {
            rb[2 * r] = 0x7fffffff;
            rb[2 * r + 1] = -1;
        }
    }
}

__global__ __launch_bounds__(256) void k_cc_rows(const int* __restrict__ L, int W, long HW, long LH, const int* __restrict__ cy0,
                                                 const int* __restrict__ crow, int* __restrict__ row, long C, long rowcap) {
    const int b = blockIdx.y;
    const int* Lb = L + (size_t)b * LH;
    for (int k = 0; k < CHUNK / 256; ++k) {
        const long p = (long)blockIdx.x * CHUNK + k * 256 + threadIdx.x;
        if (p >= HW || Lb[p] == -1) continue;
        const int x = (int)(p % W), y = (int)(p / W);
        const bool left = x == 0 || Lb[p - 1] == -1, right = x == W - 1 || Lb[p + 1] == -1;
        if (!left && !right) continue;
        const int id = cc_id(Lb, p);
        if (!id_ok(id, C)) continue;
        const long slot = (long)crow[(size_t)b * C + id] + (y - cy0[(size_t)b * C + id]);
        if (slot >= rowcap) continue;
        int* r = row + ((size_t)b * rowcap + slot) * 2;
        if (left) atomicMin(r, x);
        if (right) atomicMax(r + 1, x);
    }
}

// np.hypot of the host = glibc's hypot (the non-FMA correction kernel; edge vectors are integers, so no scaling branch applies)
__device__ __forceinline__ double host_hypot(double x, double y) {
    x = fabs(x);
    y = fabs(y);
    const double ax = x < y ? y : x, ay = x < y ? x : y;
    if (ay == 0.0) return ax;
    double h = sqrt(ax * ax + ay * ay), t1, t2;
    if (h <= 2.0 * ay) {
        const double d = h - ay;
        t1 = ax * (2.0 * d - ax);
        t2 = (d - 2.0 * (ax - ay)) * d;
    } else {
        const double d = h - ax;
        t1 = 2.0 * d * (ax - 2.0 * ay);
        t2 = (4.0 * d - ay) * ay + d * d;
    }
    return h - (t1 + t2) / (2.0 * h);
}

// One thread per component.  Points = the row extremes in (y, x) order; Andrew's monotone chain over them gives the host _hull's
// vertex set (collinear points dropped, same orientation); rotated to start at the lexicographically smallest (x, y) vertex it is the
// host's sequence.  The stack lives in the component's slice of the (now dead) label array: 2h + 2 slots, encoded (row << 1 | side).
__global__ __launch_bounds__(256) void k_cc_quad(const int* __restrict__ ncomp, const int* __restrict__ cy0, const int* __restrict__ cy1,
                                                 const int* __restrict__ crow, const int* __restrict__ row, int* __restrict__ L, long LH, long C,
                                                 long rowcap, float* __restrict__ quads) {
    const int b = blockIdx.y;
    const long n_c = min((long)ncomp[b], C);
    for (long id = (long)blockIdx.x * 256 + threadIdx.x; id < n_c; id += (long)gridDim.x * 256) {
        const int y0 = cy0[(size_t)b * C + id], h = cy1[(size_t)b * C + id] - y0 + 1;
        const long ro = crow[(size_t)b * C + id];
        float* q = quads + ((size_t)b * C + id) * 8;
        if (ro + h > rowcap) {  // cannot happen (sum of heights <= H * ceil(W / 2)); leave a NaN quad rather than read out of range
            for (int i = 0; i < 8; ++i) q[i] = __int_as_float(0x7fc00000);
            continue;
        }
        const int* R = row + ((size_t)b * rowcap + ro) * 2;
        int* S = L + (size_t)b * LH + 2 * ro + 2 * id;
        auto PX = [&](int e) -> long long { return R[e]; };  // e = (row << 1) | side indexes R directly
        auto PY = [&](int e) -> long long { return y0 + (e >> 1); };
        auto cross = [&](int a, int c, int p) {
            return (PX(c) - PX(a)) * (PY(p) - PY(a)) - (PY(c) - PY(a)) * (PX(p) - PX(a));
        };
        int npts = 0;
        for (int r = 0; r < h; ++r) npts += 1 + (R[2 * r + 1] != R[2 * r]);
        int v = 0;
        if (npts <= 2) {
            for (int r = 0; r < h; ++r) {
                S[v++] = 2 * r;
                if (R[2 * r + 1] != R[2 * r]) S[v++] = 2 * r + 1;
            }
        } else {
            int k = 0;
            for (int r = 0; r < h; ++r)
                for (int sd = 0; sd < 1 + (R[2 * r + 1] != R[2 * r]); ++sd) {
                    const int e = 2 * r + sd;
                    while (k >= 2 && cross(S[k - 2], S[k - 1], e) <= 0) --k;
                    S[k++] = e;
                }
            const int t = k + 1;
            bool first = true;  // the reverse pass starts at the second-to-last point
            for (int r = h - 1; r >= 0; --r)
                for (int sd = (R[2 * r + 1] != R[2 * r]); sd >= 0; --sd) {
                    if (first) {
                        first = false;
                        continue;
                    }
                    const int e = 2 * r + sd;
                    while (k >= t && cross(S[k - 2], S[k - 1], e) <= 0) --k;
                    S[k++] = e;
                }
            v = k - 1;
        }
        int s0 = 0;
        for (int i = 1; i < v; ++i)
            if (PX(S[i]) < PX(S[s0]) || (PX(S[i]) == PX(S[s0]) && PY(S[i]) < PY(S[s0]))) s0 = i;
        auto VX = [&](int i) { return (double)PX(S[(s0 + i) % v]); };
        auto VY = [&](int i) { return (double)PY(S[(s0 + i) % v]); };
        double c[8];
        if (v == 1) {
            for (int i = 0; i < 4; ++i) {
                c[2 * i] = VX(0);
                c[2 * i + 1] = VY(0);
            }
        } else if (v == 2) {
            c[0] = VX(0), c[1] = VY(0), c[2] = VX(1), c[3] = VY(1), c[4] = VX(1), c[5] = VY(1), c[6] = VX(0), c[7] = VY(0);
        } else {
            double best = 0, bux = 0, buy = 0, bx0 = 0, bx1 = 0, by0 = 0, by1 = 0;
            for (int k = 0; k < v; ++k) {
                const int k1 = k + 1 == v ? 0 : k + 1;
                const double ex = VX(k1) - VX(k), ey = VY(k1) - VY(k);
                const double len = host_hypot(ex, ey);
                const double ux = ex / len, uy = ey / len;  // edge direction; its normal is (-uy, ux)
                double x0 = 0, x1 = 0, yy0 = 0, yy1 = 0;
                for (int i = 0; i < v; ++i) {
                    const double hx = VX(i), hy = VY(i);
                    const double px = fma(hy, uy, hx * ux);      // hull @ ux.T (BLAS: fma of the second term onto the first product)
                    const double py = fma(hy, ux, hx * (-uy));   // hull @ uy.T
                    if (i == 0) {
                        x0 = x1 = px;
                        yy0 = yy1 = py;
                    } else {
                        x0 = fmin(x0, px), x1 = fmax(x1, px), yy0 = fmin(yy0, py), yy1 = fmax(yy1, py);
                    }
                }
                const double a = (x1 - x0) * (yy1 - yy0);
                if (k == 0 || a < best) {  // np.argmin: the first minimum
                    best = a, bux = ux, buy = uy, bx0 = x0, bx1 = x1, by0 = yy0, by1 = yy1;
                }
            }
            const double A[4] = {bx0, bx1, bx1, bx0}, Bv[4] = {by0, by0, by1, by1};
            for (int i = 0; i < 4; ++i) {
                c[2 * i] = A[i] * bux + Bv[i] * (-buy);
                c[2 * i + 1] = A[i] * buy + Bv[i] * bux;
            }
        }
        for (int i = 0; i < 8; ++i) q[i] = (float)c[i];
    }
}

// ------------------------------------------------------------------ box match ----------------------------------------------
__device__ __forceinline__ int bucket_of(float xmin, int nbkt) {
    if (!(xmin >= 0.0f)) return 0;
    return xmin >= (float)(nbkt - 1) ? nbkt - 1 : (int)xmin;
}

struct BmWs {
    unsigned long long* acc;  // [B][2] matches | merged
    int* maxw;                // [B] widest target bbox (float bits, >= 0)
    int* cnt;                 // [B][nbkt]: counts, then scatter cursors
    int* off;                 // [B][nbkt + 1] bucket offsets
    int* sorted;              // [B][capT] target ids by bucket
    int* split;               // [B][capT] predictions covering more than half of each target
};

__global__ __launch_bounds__(256) void k_bm_count(const float* __restrict__ tq, const int* __restrict__ nt, long capT, int nbkt, BmWs w) {
    const int b = blockIdx.y;
    const long n = min((long)nt[b], capT);
    for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < n; j += (long)gridDim.x * 256) {
        const float* q = tq + ((size_t)b * capT + j) * 8;
        float x0 = q[0], x1 = q[0];
        for (int i = 1; i < 4; ++i) x0 = fminf(x0, q[2 * i]), x1 = fmaxf(x1, q[2 * i]);
        atomicAdd(w.cnt + (size_t)b * nbkt + bucket_of(x0, nbkt), 1);
        const float wd = x1 - x0;
        atomicMax(w.maxw + b, wd > 0.0f ? __float_as_int(wd) : 0);
        w.split[(size_t)b * capT + j] = 0;
    }
}

__global__ __launch_bounds__(1024) void k_bm_scan(int nbkt, BmWs w) {
    __shared__ int s_w[16];
    const int b = blockIdx.x;
    int* c = w.cnt + (size_t)b * nbkt;
    int* o = w.off + (size_t)b * (nbkt + 1);
    for (long i = threadIdx.x; i < nbkt; i += 1024) o[i] = c[i];
    __syncthreads();
    const long tot = block_scan_excl(o, nbkt, s_w);
    __syncthreads();
    for (long i = threadIdx.x; i < nbkt; i += 1024) c[i] = o[i];  // cursors
    if (threadIdx.x == 0) o[nbkt] = (int)tot;
}

__global__ __launch_bounds__(256) void k_bm_scatter(const float* __restrict__ tq, const int* __restrict__ nt, long capT, int nbkt, BmWs w) {
    const int b = blockIdx.y;
    const long n = min((long)nt[b], capT);
    for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < n; j += (long)gridDim.x * 256) {
        const float* q = tq + ((size_t)b * capT + j) * 8;
        float x0 = q[0];
        for (int i = 1; i < 4; ++i) x0 = fminf(x0, q[2 * i]);
        const int pos = atomicAdd(w.cnt + (size_t)b * nbkt + bucket_of(x0, nbkt), 1);
        w.sorted[(size_t)b * capT + pos] = (int)j;
    }
}

__global__ __launch_bounds__(256) void k_bm_pairs(const float* __restrict__ pq, const int* __restrict__ np_, long capP, const float* __restrict__ tq,
                                                  const int* __restrict__ nt, long capT, int nbkt, BmWs w) {
    const int b = blockIdx.y;
    const long n = min((long)np_[b], capP);
    const float maxw = __int_as_float(w.maxw[b]);
    const int* o = w.off + (size_t)b * (nbkt + 1);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        double ax[4], ay[4];
        load_quad(pq + ((size_t)b * capP + i) * 8, ax, ay);
        const double pa = area_of(ax, ay, 4);
        double pminx = ax[0], pmaxx = ax[0], pminy = ay[0], pmaxy = ay[0];
        for (int k = 1; k < 4; ++k) pminx = fmin(pminx, ax[k]), pmaxx = fmax(pmaxx, ax[k]), pminy = fmin(pminy, ay[k]), pmaxy = fmax(pmaxy, ay[k]);
        // a target can pass the strict prefilter only if its x-min lies in (pminx - maxw, pmaxx): scan those buckets (one more on each side)
        const double lo = floor(pminx - (double)maxw) - 1.0, hi = floor(pmaxx) + 1.0;
        const int b0 = !(lo > 0.0) ? 0 : (lo >= nbkt - 1 ? nbkt - 1 : (int)lo);         // (a NaN bound scans from the first bucket)
        const int b1 = !(hi < nbkt - 1) ? nbkt - 1 : (hi <= 0.0 ? 0 : (int)hi);
        bool match = false;
        unsigned covered = 0;
        for (int s = o[b0]; s < o[b1 + 1]; ++s) {
            const long j = w.sorted[(size_t)b * capT + s];
            double bx[4], by[4];
            load_quad(tq + ((size_t)b * capT + j) * 8, bx, by);
            double tminx = bx[0], tmaxx = bx[0], tminy = by[0], tmaxy = by[0];
            for (int k = 1; k < 4; ++k) tminx = fmin(tminx, bx[k]), tmaxx = fmax(tmaxx, bx[k]), tminy = fmin(tminy, by[k]), tmaxy = fmax(tmaxy, by[k]);
            if (!(pminx < tmaxx && tminx < pmaxx && pminy < tmaxy && tminy < pmaxy)) continue;
            const double ta = area_of(bx, by, 4);
            if (pa == 0.0 || ta == 0.0) continue;       // intersection 0: IoU 0 / 0 and both coverages are false, as on the host
            const double inter = quad_inter(ax, ay, bx, by);
            if (!(inter > 0.0)) continue;
            const double uni = pa + ta - inter;
            match |= inter / uni > 0.5;
            covered += inter / ta > 0.5;
            if (inter / pa > 0.5) atomicAdd(w.split + (size_t)b * capT + j, 1);
        }
        if (match) atomicAdd(w.acc + 2 * b, 1ull);
        if (covered > 1) atomicAdd(w.acc + 2 * b + 1, (unsigned long long)covered);
    }
}

__global__ __launch_bounds__(1024) void k_bm_final(const int* __restrict__ np_, long capP, const int* __restrict__ nt, long capT, BmWs w,
                                                   double* __restrict__ out) {
    __shared__ int s_w[16];
    const int b = blockIdx.x;
    const long P = min((long)np_[b], capP), T = min((long)nt[b], capT);
    int cnt = 0;
    for (long j = threadIdx.x; j < T; j += 1024) cnt += w.split[(size_t)b * capT + j] > 1;
    for (int d = 32; d > 0; d >>= 1) cnt += __shfl_down(cnt, d);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x != 0) return;
    long split = 0;
    for (int k = 0; k < 16; ++k) split += s_w[k];
    const double m = (double)w.acc[2 * b], merged = (double)w.acc[2 * b + 1];
    out[4 * b + 0] = P > 0 ? m / (double)P : 1.0;
    out[4 * b + 1] = T > 0 ? m / (double)T : 1.0;
    out[4 * b + 2] = T > 0 ? merged / (double)T : 0.0;
    out[4 * b + 3] = T > 0 ? (double)split / (double)T : 0.0;
}

// ------------------------------------------------------------------ workspace layouts --------------------------------------
constexpr size_t AL = 256;
inline size_t al(size_t x) { return (x + AL - 1) / AL * AL; }

struct CcLayout {
    long HW, C, rowcap, LH, nch;
    size_t L, row, chunk, cy0, cy1, crow, bytes;
};

// per image: labels / hull stacks LH ints, row extents 2 * rowcap ints (rowcap = H * ceil(W/2) >= sum of component heights),
// chunk counts, and three ints per possible component (C = ceil(H/2) * ceil(W/2))
bool cc_layout(int B, int H, int W, CcLayout& c) {
    if (B < 1 || H < 1 || W < 1) return false;
    c.HW = (long)H * W;
    c.C = cdiv(H, 2) * cdiv(W, 2);
    c.rowcap = (long)H * cdiv(W, 2);
    c.LH = 2 * c.rowcap + 2 * c.C;
    c.nch = cdiv(c.HW, CHUNK);
    if (c.LH >= (1L << 31) - 1 || 2 * c.rowcap >= (1L << 31) - 1) return false;  // per-image indices stay 32-bit
    size_t o = 0;
    c.L = o, o += al((size_t)B * c.LH * 4);
    c.row = o, o += al((size_t)B * c.rowcap * 8);
    c.chunk = o, o += al((size_t)B * c.nch * 4);
    c.cy0 = o, o += al((size_t)B * c.C * 4);
    c.cy1 = o, o += al((size_t)B * c.C * 4);
    c.crow = o, o += al((size_t)B * c.C * 4);
    c.bytes = o;
    return true;
}

struct BmLayout {
    size_t acc, maxw, cnt, zero_bytes, off, sorted, split, bytes;
};

bool bm_layout(int B, long capT, int nbkt, BmLayout& l) {
    if (B < 1 || capT < 0 || nbkt < 1 || capT >= (1L << 31) - 1) return false;
    size_t o = 0;
    l.acc = o, o += (size_t)B * 16;
    l.maxw = o, o += (size_t)B * 4;
    l.cnt = o, o += (size_t)B * nbkt * 4;
    l.zero_bytes = o;
    o = al(o);
    l.off = o, o += al((size_t)B * (nbkt + 1) * 4);
    l.sorted = o, o += al((size_t)B * capT * 4);
    l.split = o, o += al((size_t)B * capT * 4);
    l.bytes = o;
    return true;
}

int grid_for(long n) { return (int)max(1L, min(cdiv(n, 256), 64L)); }

int cc_quads(const void* mask, int kind, float thr, int B, int H, int W, int* ncomp, float* quads, int* labels, void* ws, hipStream_t st) {
    CcLayout c;
    OCRS_CHECK_ARG(mask && ncomp && quads && ws && (kind == 0 || kind == 1) && cc_layout(B, H, W, c));
    OCRS_CHECK_ARG(B <= 65535);
    char* base = static_cast<char*>(ws);
    int* L = reinterpret_cast<int*>(base + c.L);
    int* row = reinterpret_cast<int*>(base + c.row);
    int* chunk = reinterpret_cast<int*>(base + c.chunk);
    int* cy0 = reinterpret_cast<int*>(base + c.cy0);
    int* cy1 = reinterpret_cast<int*>(base + c.cy1);
    int* crow = reinterpret_cast<int*>(base + c.crow);
    const int tilesX = (int)cdiv(W, TW), tiles = tilesX * (int)cdiv(H, TH);
    const dim3 gt(tiles, B), gc((unsigned)c.nch, B);
    if (kind == 0)
        k_cc_local<0><<<gt, 256, 0, st>>>(mask, thr, L, H, W, c.LH, tilesX);
    else
        k_cc_local<1><<<gt, 256, 0, st>>>(mask, thr, L, H, W, c.LH, tilesX);
    k_cc_border<<<gt, 128, 0, st>>>(L, H, W, c.LH, tilesX);
    k_cc_flatten<<<gc, 256, 0, st>>>(L, c.HW, c.LH, chunk, (int)c.nch);
    k_scan_chunks<<<B, 1024, 0, st>>>(chunk, c.nch, ncomp);
    k_cc_number<<<gc, 256, 0, st>>>(L, W, c.HW, c.LH, chunk, (int)c.nch, cy0, cy1, c.C);
    if (labels) k_cc_labels<<<gc, 256, 0, st>>>(L, c.HW, c.LH, labels);
    k_cc_ymax<<<gc, 256, 0, st>>>(L, W, c.HW, c.LH, cy1, c.C);
    k_cc_rowoff<<<B, 1024, 0, st>>>(ncomp, cy0, cy1, crow, row, c.C, c.rowcap);
    k_cc_rows<<<gc, 256, 0, st>>>(L, W, c.HW, c.LH, cy0, crow, row, c.C, c.rowcap);
    k_cc_quad<<<dim3(grid_for(c.C), B), 256, 0, st>>>(ncomp, cy0, cy1, crow, row, L, c.LH, c.C, c.rowcap, quads);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

int box_match(const float* pq, const int* np_, long capP, const float* tq, const int* nt, long capT, int B, int nbkt, double* out, void* ws,
              hipStream_t st) {
    BmLayout l;
    OCRS_CHECK_ARG(pq && np_ && tq && nt && out && ws && capP >= 0 && capP < (1L << 31) - 1 && bm_layout(B, capT, nbkt, l) && B <= 65535);
    char* base = static_cast<char*>(ws);
    BmWs w{reinterpret_cast<unsigned long long*>(base + l.acc), reinterpret_cast<int*>(base + l.maxw), reinterpret_cast<int*>(base + l.cnt),
           reinterpret_cast<int*>(base + l.off), reinterpret_cast<int*>(base + l.sorted), reinterpret_cast<int*>(base + l.split)};
    if (hipMemsetAsync(ws, 0, l.zero_bytes, st) != hipSuccess) return OCRS_ERR_HIP;
    k_bm_count<<<dim3(grid_for(capT), B), 256, 0, st>>>(tq, nt, capT, nbkt, w);
    k_bm_scan<<<B, 1024, 0, st>>>(nbkt, w);
    k_bm_scatter<<<dim3(grid_for(capT), B), 256, 0, st>>>(tq, nt, capT, nbkt, w);
    k_bm_pairs<<<dim3(grid_for(capP), B), 256, 0, st>>>(pq, np_, capP, tq, nt, capT, nbkt, w);
    k_bm_final<<<B, 1024, 0, st>>>(np_, capP, nt, capT, w, out);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

struct MmLayout {
    CcLayout cc;
    BmLayout bm;
    size_t qp, qt, np_, nt, bmws, bytes;
};

bool mm_layout(int B, int H, int W, MmLayout& m) {
    if (!cc_layout(B, H, W, m.cc) || !bm_layout(B, m.cc.C, W, m.bm)) return false;
    size_t o = al(m.cc.bytes);
    m.qp = o, o += al((size_t)B * m.cc.C * 32);
    m.qt = o, o += al((size_t)B * m.cc.C * 32);
    m.np_ = o, o += al((size_t)B * 4);
    m.nt = o, o += al((size_t)B * 4);
    m.bmws = o, o += al(m.bm.bytes);
    m.bytes = o;
    return true;
}

}  // namespace

extern "C" {

long ocrs_cc_quads_capacity(int H, int W) { return H < 1 || W < 1 ? 0 : cdiv(H, 2) * cdiv(W, 2); }

long ocrs_cc_quads_ws_bytes(int B, int H, int W) {
    CcLayout c;
    return cc_layout(B, H, W, c) ? (long)c.bytes : 0;
}

int ocrs_cc_quads(const void* mask, int kind, float threshold, int B, int H, int W, int* ncomp, float* quads, int* labels, void* ws,
                  hipStream_t st) {
    return cc_quads(mask, kind, threshold, B, H, W, ncomp, quads, labels, ws, st);
}

long ocrs_box_match_ws_bytes(int B, long cap_t, int nbkt) {
    BmLayout l;
    return bm_layout(B, cap_t, nbkt, l) ? (long)l.bytes : 0;
}

int ocrs_box_match_metrics(const float* pred_quads, const int* n_pred, long cap_p, const float* target_quads, const int* n_target, long cap_t, int B,
                           int nbkt, double* out, void* ws, hipStream_t st) {
    return box_match(pred_quads, n_pred, cap_p, target_quads, n_target, cap_t, B, nbkt, out, ws, st);
}

long ocrs_mask_metrics_ws_bytes(int B, int H, int W) {
    MmLayout m;
    return mm_layout(B, H, W, m) ? (long)m.bytes : 0;
}

int ocrs_mask_metrics(const void* pred, int pred_kind, const void* target, int target_kind, float threshold, int B, int H, int W, double* out, void* ws,
                      hipStream_t st) {
    MmLayout m;
    OCRS_CHECK_ARG(pred && target && out && ws && mm_layout(B, H, W, m));
    char* base = static_cast<char*>(ws);
    float* qp = reinterpret_cast<float*>(base + m.qp);
    float* qt = reinterpret_cast<float*>(base + m.qt);
    int* np_ = reinterpret_cast<int*>(base + m.np_);
    int* nt = reinterpret_cast<int*>(base + m.nt);
    int r = cc_quads(pred, pred_kind, threshold, B, H, W, np_, qp, nullptr, ws, st);  // the labelling workspace is reused by the second side
    if (r == OCRS_OK) r = cc_quads(target, target_kind, threshold, B, H, W, nt, qt, nullptr, ws, st);
    if (r == OCRS_OK) r = box_match(qp, np_, m.cc.C, qt, nt, m.cc.C, B, W, out, base + m.bmws, st);
    return r;
}

}  // extern "C"
