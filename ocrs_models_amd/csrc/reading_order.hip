// Reading order: the text lines of every page put into the order a reader takes them, column by column, and split into blocks, by one
// deterministic geometric rule after Breuel's two ordering criteria (DESIGN.md §16 states it; the numpy restatement is
// tests/reading_ref.py).  Runs after the line stage of text_lines.hip on its line quads; every count stays on the device.
//
//   k_read_clear      before[cap][pitch] = 0: rows and columns from L on and bits between pages stay 0
//   k_read_page_scan  blk_offs [B + 1]: exclusive scan of ceil(L_p / 256), the row tiles of each page; one workgroup
//   k_read_extents    one wave per page: U = normalise(sum of lng_l * u_l in line order), then one lane per line projects the four corners
//                     on U, V -> ext [L][8] = x0, x1, y0, y1, yc, sht, 0, 0
//   k_read_relation   workgroup = (256 rows of one page, one 32-bit column word): lane a builds the word of before(a, b) for its 32 columns b,
//                     the b and the blocker candidates c read from LDS by broadcast; one lane stores one word
//   k_read_peel       one workgroup per page: in-degrees = column popcounts, then L_p rounds of (workgroup minimum, emit, decrement)
//   k_read_blocks     one lane per position: new_block
//
// A single page is B = 1 with line_page_offs == NULL: its lines are 0 .. L.  All decision arithmetic is fp32 with one rounding per operation
// (no fused multiply-add), so the restatement follows it operation by operation.  No atomics at all.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kTile = 256;         // rows of a relation workgroup, and the lines staged in LDS per step of the blocker walk
constexpr int kPeelLdsMax = 2048;  // in-degrees of a page in LDS up to here (8 KB), in the workspace above
constexpr int kForced = 1 << 30;   // key offset of a line that is unemitted but still has unemitted lines before it
constexpr long kMaxLines = 1L << 15;  // before is cap * ceil(cap / 32) words: 128 MB here
constexpr int kMaxPages = 1 << 20;

// ws layout (ocrs_reading_order_ws_bytes)
struct ReadWs {
    float* ext;     // [cap][8]: x0, x1, y0, y1, yc, sht, 0, 0
    int* deg;       // [cap] in-degrees of the pages that do not fit LDS
    int* blk_offs;  // [B + 1] first relation row tile of every page
};
inline long ws_cap(long n) { return (n + 3) & ~3L; }
inline ReadWs ws_split(void* ws, long cap) {
    ReadWs w;
    char* p = static_cast<char*>(ws);
    w.ext = reinterpret_cast<float*>(p), p += ws_cap(cap) * 32;
    w.deg = reinterpret_cast<int*>(p), p += ws_cap(cap) * 4;
    w.blk_offs = reinterpret_cast<int*>(p);
    return w;
}
inline long pitch_of(long cap) { return (cap + 31) / 32; }

__device__ __forceinline__ int line_count(const int* __restrict__ n_lines, long cap) { return (int)min((long)max(*n_lines, 0), cap); }
// line range of page p, clamped so that offsets that are no ascending scan still index inside the L lines; offs == NULL: the one page is 0 .. L
__device__ __forceinline__ int2 page_range(const int* __restrict__ offs, int p, int L) {
    if (!offs) return make_int2(0, L);
    const int lo = min(max(offs[p], 0), L);
    return make_int2(lo, min(max(offs[p + 1], lo), L));
}
// the last p in [0, B) with offs[p] <= k (offs ascending, offs[0] <= k): the page of row tile k in blk_offs, of position k in line_page_offs
__device__ __forceinline__ int last_le(const int* __restrict__ offs, int B, int k) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (offs[mid] <= k) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_read_clear(unsigned* __restrict__ before, long words) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < words) before[i] = 0u;
}

// One workgroup: blk_offs[0..B] = exclusive scan over the pages, 256 at a time, of ceil(L_p / kTile).
__global__ __launch_bounds__(256) void k_read_page_scan(const int* __restrict__ n_lines, long cap, const int* __restrict__ offs, int B, int* __restrict__ blk_offs) {
    __shared__ int s_scan[256];
    const int L = line_count(n_lines, cap);
    const int t = threadIdx.x;
    int base = 0;
    for (int p0 = 0; p0 < B; p0 += 256) {
        const int p = p0 + t;
        int v = 0;
        if (p < B) {
            const int2 r = page_range(offs, p, L);
            v = (r.y - r.x + kTile - 1) / kTile;
        }
        __syncthreads();
        s_scan[t] = v;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {
            const int add = t >= o ? s_scan[t - o] : 0;
            __syncthreads();
            s_scan[t] += add;
            __syncthreads();
        }
        if (p < B) blk_offs[p] = base + s_scan[t] - v;
        base += s_scan[255];
    }
    if (t == 0) blk_offs[B] = base;
}

// ---- page axis and extents ---------------------------------------------------------------------------------------------------------
// The frame of a line quad by the word-frame rule of text_lines.hip (longer side, tie -> larger |x|, sign so that u.x > 0 or u.x == 0 and
// u.y > 0), kept as this file's own text so that neither can change the other's bits.
struct Frame {
    float ux, uy, lng, sht;
};
__device__ __forceinline__ Frame line_frame(float4 a, float4 c) {
    const float e1x = a.z - a.x, e1y = a.w - a.y, e2x = c.x - a.z, e2y = c.y - a.w;
    const float l1 = sqrtf(e1x * e1x + e1y * e1y), l2 = sqrtf(e2x * e2x + e2y * e2y);
    const bool first = l1 > l2 || (l1 == l2 && fabsf(e1x) >= fabsf(e2x));
    Frame f;
    f.lng = first ? l1 : l2, f.sht = first ? l2 : l1;
    f.ux = 1.0f, f.uy = 0.0f;
    if (f.lng > 0.0f) f.ux = (first ? e1x : e2x) / f.lng, f.uy = (first ? e1y : e2y) / f.lng;
    if (f.ux < 0.0f || (f.ux == 0.0f && f.uy < 0.0f)) f.ux = -f.ux, f.uy = -f.uy;
    return f;
}
// One wave per page.  The direction sum takes the lines one after the other in line order (lane k of a chunk of 64 holds line k's term; the
// running sum takes them by lane index, so every lane holds the same bits).  Then lane k of every chunk projects line k's corners.
__global__ __launch_bounds__(256) void k_read_extents(const float* __restrict__ quads, const int* __restrict__ n_lines, long cap, const int* __restrict__ offs, int B,
                                                      float* __restrict__ ext) {
    const int L = line_count(n_lines, cap);
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= B) return;  // (wave-uniform)
    const int2 r = page_range(offs, p, L);
    float sx = 0.0f, sy = 0.0f;
    for (int l0 = r.x; l0 < r.y; l0 += 64) {
        float wx = 0.0f, wy = 0.0f;
        if (l0 + lane < r.y) {
            const Frame f = line_frame(reinterpret_cast<const float4*>(quads)[2 * (long)(l0 + lane)], reinterpret_cast<const float4*>(quads)[2 * (long)(l0 + lane) + 1]);
            wx = f.lng * f.ux, wy = f.lng * f.uy;
        }
        const int m = min(64, r.y - l0);
        for (int q = 0; q < m; ++q) sx = sx + __shfl(wx, q, 64), sy = sy + __shfl(wy, q, 64);
    }
    const float norm = sqrtf(sx * sx + sy * sy);
    float ux = 1.0f, uy = 0.0f;
    if (norm > 0.0f) ux = sx / norm, uy = sy / norm;
    const float vx = -uy, vy = ux;
    for (int l = r.x + lane; l < r.y; l += 64) {
        const float4 a = reinterpret_cast<const float4*>(quads)[2 * (long)l], c = reinterpret_cast<const float4*>(quads)[2 * (long)l + 1];
        const Frame f = line_frame(a, c);
        const float xs[4] = {a.x, a.z, c.x, c.z}, ys[4] = {a.y, a.w, c.y, c.w};
        float pu[4], pv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) pu[q] = xs[q] * ux + ys[q] * uy, pv[q] = xs[q] * vx + ys[q] * vy;
        const float x0 = fminf(fminf(pu[0], pu[1]), fminf(pu[2], pu[3])), x1 = fmaxf(fmaxf(pu[0], pu[1]), fmaxf(pu[2], pu[3]));
        const float y0 = fminf(fminf(pv[0], pv[1]), fminf(pv[2], pv[3])), y1 = fmaxf(fmaxf(pv[0], pv[1]), fmaxf(pv[2], pv[3]));
        const float yc = 0.25f * ((pv[0] + pv[1]) + (pv[2] + pv[3]));
        reinterpret_cast<float4*>(ext)[2 * (long)l] = make_float4(x0, x1, y0, y1);
        reinterpret_cast<float4*>(ext)[2 * (long)l + 1] = make_float4(yc, f.sht, 0.0f, 0.0f);
    }
}

// ---- relation ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool overlap(float x0a, float x1a, float x0b, float x1b) { return fminf(x1a, x1b) > fmaxf(x0a, x0b); }

// Workgroup (k, wl): row tile k belongs to page p (bisecting blk_offs, as k_line_links_pages finds its page), lane t is row
// a = lo + (k - blk_offs[p]) * 256 + t, and the workgroup's column word is w = (lo >> 5) + wl, columns 32 w .. 32 w + 31 cut to [lo, hi).
// Pass 1 decides rule 1 and the left-of test of rule 2 for the 32 columns (their extents in LDS, one address per step: a broadcast) and
// notes the pairs that hold unless blocked.  Pass 2 walks the page's lines c, staged 256 at a time, for every such pair; a column that no
// lane of the wave still has pending is skipped (wave-uniform).  c == a and c == b fail the strict yc test by themselves.
__global__ __launch_bounds__(kTile) void k_read_relation(const float* __restrict__ ext, const int* __restrict__ n_lines, long cap, const int* __restrict__ offs,
                                                         const int* __restrict__ blk_offs, int B, unsigned* __restrict__ before, int pitch) {
    __shared__ float4 s_b[32];     // x0, x1, yc, 0 of the 32 columns
    __shared__ float4 s_c[kTile];  // the same of a tile of blocker candidates
    const int L = line_count(n_lines, cap);
    const int k = blockIdx.x;
    if (k >= blk_offs[B]) return;  // (block-uniform)
    const int p = last_le(blk_offs, B, k);
    const int2 r = page_range(offs, p, L);
    const int w = (r.x >> 5) + (int)blockIdx.y;
    if (r.y <= r.x || w > ((r.y - 1) >> 5)) return;  // (block-uniform)
    const int t = threadIdx.x, a = r.x + (k - blk_offs[p]) * kTile + t;
    const bool row = a < r.y;
    const int b_lo = max(w << 5, r.x), b_hi = min((w << 5) + 32, r.y);  // b_lo < b_hi <= L
    if (t < 32) {
        const int b = (w << 5) + t;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (b >= b_lo && b < b_hi) {
            const float4 e = reinterpret_cast<const float4*>(ext)[2 * (long)b];
            v = make_float4(e.x, e.y, ext[8 * (long)b + 4], 0.0f);
        }
        s_b[t] = v;
    }
    float x0a = 0.0f, x1a = 0.0f, yca = 0.0f;
    if (row) {
        const float4 e = reinterpret_cast<const float4*>(ext)[2 * (long)a];
        x0a = e.x, x1a = e.y, yca = ext[8 * (long)a + 4];
    }
    __syncthreads();
    unsigned word = 0u, pend = 0u;
    if (row) {
        for (int b = b_lo; b < b_hi; ++b) {
            const float4 eb = s_b[b & 31];
            if (b == a) continue;
            if (overlap(x0a, x1a, eb.x, eb.y)) {
                if (yca < eb.z || (yca == eb.z && a < b)) word |= 1u << (b & 31);
            } else if (x1a <= eb.x) {
                pend |= 1u << (b & 31);
            }
        }
    }
    for (int c0 = r.x; c0 < r.y; c0 += kTile) {
        const int m = min(kTile, r.y - c0);
        __syncthreads();
        if (t < m) {
            const float4 e = reinterpret_cast<const float4*>(ext)[2 * (long)(c0 + t)];
            s_c[t] = make_float4(e.x, e.y, ext[8 * (long)(c0 + t) + 4], 0.0f);
        }
        __syncthreads();
        for (int b = b_lo; b < b_hi; ++b) {
            const bool need = (pend >> (b & 31)) & 1u;
            if (!__any(need)) continue;
            const float4 eb = s_b[b & 31];
            const float lo = fminf(yca, eb.z), hi = fmaxf(yca, eb.z);
            bool blocked = false;
#pragma unroll 4
            for (int q = 0; q < m; ++q) {
                const float4 ec = s_c[q];
                blocked = blocked || (lo < ec.z && ec.z < hi && overlap(ec.x, ec.y, x0a, x1a) && overlap(ec.x, ec.y, eb.x, eb.y));
            }
            if (need && blocked) pend &= ~(1u << (b & 31));
        }
    }
    if (row) before[(long)a * pitch + w] = word | pend;
}

// ---- peel --------------------------------------------------------------------------------------------------------------------------
// One workgroup per page.  deg[j] = number of unemitted lines before line j (a column popcount), -1 once j is emitted.  A round: every lane
// offers the smallest of its lines with deg == 0, or else the smallest unemitted one raised by kForced; the workgroup minimum e is emitted;
// every line j with bit (e, j) loses one.  Exactly L_p - k lines are unemitted in round k, so e is always a line of the page.
__global__ __launch_bounds__(256) void k_read_peel(const int* __restrict__ n_lines, long cap, const int* __restrict__ offs, int B, const unsigned* __restrict__ before,
                                                   int pitch, int* __restrict__ line_order, int* __restrict__ ws_deg) {
    __shared__ int s_deg[kPeelLdsMax];
    __shared__ int s_min[4];
    const int L = line_count(n_lines, cap);
    const int2 r = page_range(offs, blockIdx.x, L);
    const int n = r.y - r.x, t = threadIdx.x;
    if (n <= 0) return;  // (block-uniform)
    int* deg = n <= kPeelLdsMax ? s_deg : ws_deg + r.x;
    for (int j = t; j < n; j += 256) {
        const int col = r.x + j;
        int d = 0;
        for (int a = r.x; a < r.y; ++a) d += (before[(long)a * pitch + (col >> 5)] >> (col & 31)) & 1u;
        deg[j] = d;
    }
    __syncthreads();
    for (int k = 0; k < n; ++k) {
        int key = 0x7fffffff;
        for (int j = t; j < n; j += 256) {
            const int d = deg[j];
            if (d == 0) {
                key = min(key, j);
                break;  // (this lane's lines ascend)
            }
            if (d > 0) key = min(key, j + kForced);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) key = min(key, __shfl_xor(key, o, 64));
        if ((t & 63) == 0) s_min[t >> 6] = key;
        __syncthreads();
        key = min(min(s_min[0], s_min[1]), min(s_min[2], s_min[3]));
        const int e = key >= kForced ? key - kForced : key;
        if ((unsigned)e >= (unsigned)n) return;  // (never: block-uniform)
        if (t == 0) line_order[r.x + k] = r.x + e;
        const unsigned* __restrict__ row = before + (long)(r.x + e) * pitch;
        for (int j = t; j < n; j += 256) {
            const int d = deg[j];
            if (j == e) deg[j] = -1;
            else if (d > 0 && ((row[(r.x + j) >> 5] >> ((r.x + j) & 31)) & 1u)) deg[j] = d - 1;
        }
        __syncthreads();
    }
}

// ---- blocks ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_read_blocks(const float* __restrict__ ext, const int* __restrict__ n_lines, long cap, const int* __restrict__ offs, int B,
                                                     float block_gap, const int* __restrict__ line_order, int* __restrict__ new_block) {
    const int L = line_count(n_lines, cap);
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= L) return;
    const int2 r = page_range(offs, offs ? last_le(offs, B, k) : 0, L);
    int flag = 1;
    if (k > r.x && k < r.y) {
        const int p = line_order[k - 1], q = line_order[k];
        if (p >= r.x && p < r.y && q >= r.x && q < r.y && p != q) {
            const float4 ep = reinterpret_cast<const float4*>(ext)[2 * (long)p], eq = reinterpret_cast<const float4*>(ext)[2 * (long)q];
            const float2 fp = *reinterpret_cast<const float2*>(ext + 8 * (long)p + 4), fq = *reinterpret_cast<const float2*>(ext + 8 * (long)q + 4);
            const bool rule1 = overlap(ep.x, ep.y, eq.x, eq.y) && (fp.x < fq.x || (fp.x == fq.x && p < q));
            const bool near = eq.z - ep.w <= block_gap * fmaxf(fp.y, fq.y);
            flag = (rule1 && near) ? 0 : 1;
        }
    }
    new_block[k] = flag;
}

inline unsigned blocks(long n, int per) { return (unsigned)((n + per - 1) / per); }
inline bool sizes_ok(long cap, int B) { return cap >= 0 && cap <= kMaxLines && B >= 0 && B <= kMaxPages; }

}  // namespace

extern "C" {

long ocrs_reading_order_ws_bytes(long cap, int B) {
    return cap > 0 && cap <= kMaxLines && B > 0 && B <= kMaxPages ? ws_cap(cap) * 36 + ws_cap(B + 1) * 4 : 0;
}

int ocrs_reading_relation(const float* line_quads, const int* n_lines, const int* line_page_offs, int B, long cap, unsigned* before, void* ws, long ws_bytes,
                          hipStream_t st) {
    OCRS_CHECK_ARG(sizes_ok(cap, B) && (line_page_offs || B <= 1));
    if (cap == 0 || B == 0) return OCRS_OK;
    OCRS_CHECK_ARG(line_quads && n_lines && before && ws && aligned16(line_quads) && aligned16(ws) && ws_bytes >= ocrs_reading_order_ws_bytes(cap, B));
    const ReadWs w = ws_split(ws, cap);
    const int pitch = (int)pitch_of(cap);
    hipLaunchKernelGGL(k_read_clear, dim3(blocks(cap * pitch, 256)), dim3(256), 0, st, before, cap * pitch);
    hipLaunchKernelGGL(k_read_page_scan, dim3(1), dim3(256), 0, st, n_lines, cap, line_page_offs, B, w.blk_offs);
    hipLaunchKernelGGL(k_read_extents, dim3(blocks(B, 4)), dim3(256), 0, st, line_quads, n_lines, cap, line_page_offs, B, w.ext);
    hipLaunchKernelGGL(k_read_relation, dim3(blocks(cap, kTile) + (unsigned)B, (unsigned)pitch), dim3(kTile), 0, st, (const float*)w.ext, n_lines, cap, line_page_offs,
                       (const int*)w.blk_offs, B, before, pitch);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

int ocrs_reading_peel(const int* n_lines, const int* line_page_offs, int B, long cap, const unsigned* before, int* line_order, void* ws, long ws_bytes,
                      hipStream_t st) {
    OCRS_CHECK_ARG(sizes_ok(cap, B) && (line_page_offs || B <= 1));
    if (cap == 0 || B == 0) return OCRS_OK;
    OCRS_CHECK_ARG(n_lines && before && line_order && ws && aligned16(ws) && ws_bytes >= ocrs_reading_order_ws_bytes(cap, B));
    const ReadWs w = ws_split(ws, cap);
    hipLaunchKernelGGL(k_read_peel, dim3((unsigned)B), dim3(256), 0, st, n_lines, cap, line_page_offs, B, before, (int)pitch_of(cap), line_order, w.deg);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

int ocrs_reading_blocks(const int* n_lines, const int* line_page_offs, int B, long cap, float block_gap, const int* line_order, int* new_block, void* ws,
                        long ws_bytes, hipStream_t st) {
    OCRS_CHECK_ARG(sizes_ok(cap, B) && (line_page_offs || B <= 1));
    if (cap == 0 || B == 0) return OCRS_OK;
    OCRS_CHECK_ARG(n_lines && line_order && new_block && ws && aligned16(ws) && ws_bytes >= ocrs_reading_order_ws_bytes(cap, B));
    const ReadWs w = ws_split(ws, cap);
    hipLaunchKernelGGL(k_read_blocks, dim3(blocks(cap, 256)), dim3(256), 0, st, (const float*)w.ext, n_lines, cap, line_page_offs, B, block_gap, line_order, new_block);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

}  // extern "C"
