// Text lines: detected word quads grouped into reading-order lines by one deterministic geometric rule (DESIGN.md §14 states it; the
// numpy restatement is tests/lines_ref.py).  Runs between detection and recognition; every count stays on the device.
//
//   k_line_frames    per word: centre, unit long axis u, side lengths -> frames [N][8]; clears the acceptance and line tables
//   k_line_links     one lane per word i, the j frames staged 256 at a time in LDS; best (s, j) per lane; 64-bit atomicMin acceptance
//   k_line_resolve   keeps the links that were chosen AND accepted -> next_word; start state of the pointer jumping
//   k_line_rank_lds  head, rank and line length by pointer jumping in LDS, one workgroup          (N <= kRankLdsMax)
//   k_line_jump / k_line_rank_finish   the same, one launch per round through global ping-pong buffers  (N >  kRankLdsMax)
//   k_line_order     line index = counting rank of each head among the heads under (c.y, c.x, word index)
//   k_line_scan      number of lines and the exclusive scan of their lengths -> line_offsets; one workgroup
//   k_line_scatter   word_order and line_of_word
//   k_line_quads     one wave per line: direction sum in chain order, min / max of the projections by wave reduction
//
// Page batches: the words of B pages in one flat array, page p's at word_offs[p] .. word_offs[p + 1].  A word's candidates are
// the words of its own page and lines are ordered by (page, c.y, c.x, word index); frames, resolve, rank, scan, scatter and quads run unchanged
// on the flat array with the total word_offs[B] as their device count.
//   k_pages_init         chosen = -1, line_idx = 0 (words that no page covers stay in bounds), per-page head counters = 0
//   k_page_scan          blk_offs [B + 1]: exclusive scan of ceil(n_p / 256), the workgroups of each page; one workgroup
//   k_line_links_pages   k_line_links with one page per workgroup: only that page's frames are staged
//   k_line_order_pages   k_line_order likewise -> rank of each head among its page's heads, heads counted per page
//   k_page_scan          (again) line_page_offs [B + 1]: exclusive scan of the head counts
//   k_line_place_pages   line index = line_page_offs[page] + rank in the page; len_sorted, head_of_line, page_of_line
// The two links kernels share their walk, nearest_follower() over a word range [lo, hi): k_line_links passes [0, n), the paged kernel its
// workgroup's page; they differ only in how they find the range.  The two order kernels are still two texts of one count (see k_line_order_pages).
//
// All decision arithmetic is fp32 with one rounding per operation (no fused multiply-add), so the restatement follows it operation by
// operation.  No float atomics: the only atomic is an integer minimum whose result does not depend on the order of arrival.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kTile = 256;         // words staged in LDS per step of k_line_links / k_line_order
constexpr int kRankLdsMax = 2048;  // two ping-pong (pointer, distance) pairs of ints: 16 B per word = 32 KB of the 64 KB a workgroup may hold
constexpr unsigned long long kNoAccept = ~0ULL;

// ws layout (ocrs_text_lines_ws_bytes): every array has `cap` entries and starts 16-byte aligned because cap is rounded up to 4
struct LinesWs {
    float* frames;               // [cap][8]: cx, cy, ux, uy, lng, sht, 0, 0
    unsigned long long* accept;  // [cap]: min over the choosers k of (bits(s_kj) << 32 | k)
    int *chosen, *head, *rank, *len, *line_idx, *len_sorted, *head_of_line;
    int *pa, *da, *pb, *db;      // pointer jumping ping-pong
};
inline long ws_cap(long cap) { return (cap + 3) & ~3L; }
inline LinesWs ws_split(void* ws, long cap) {
    const long c = ws_cap(cap);
    LinesWs w;
    char* p = static_cast<char*>(ws);
    w.frames = reinterpret_cast<float*>(p), p += c * 32;
    w.accept = reinterpret_cast<unsigned long long*>(p), p += c * 8;
    int** arrays[] = {&w.chosen, &w.head, &w.rank, &w.len, &w.line_idx, &w.len_sorted, &w.head_of_line, &w.pa, &w.da, &w.pb, &w.db};
    for (int** a : arrays) *a = reinterpret_cast<int*>(p), p += c * 4;
    return w;
}
constexpr long kWsBytesPerWord = 32 + 8 + 11 * 4;

__device__ __forceinline__ int word_count(const int* __restrict__ count, long cap) { return (int)(count ? min((long)max(*count, 0), cap) : cap); }

// ---- word frame ------------------------------------------------------------------------------------------------------------------
// The same choice of axes as crop_frame() of crop_frame.h (longer side, tie -> larger |x|, sign so that u.x > 0 or u.x == 0 and u.y > 0),
// kept as this file's own text so that neither can change the other's bits.
__global__ __launch_bounds__(256) void k_line_frames(const float* __restrict__ quads, const int* __restrict__ count, long cap, float* __restrict__ frames,
                                                     unsigned long long* __restrict__ accept, int* __restrict__ len_sorted, int* __restrict__ head_of_line) {
    const int n = word_count(count, cap);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 a = reinterpret_cast<const float4*>(quads)[2 * (long)i], c = reinterpret_cast<const float4*>(quads)[2 * (long)i + 1];
    const float e1x = a.z - a.x, e1y = a.w - a.y, e2x = c.x - a.z, e2y = c.y - a.w;
    const float l1 = sqrtf(e1x * e1x + e1y * e1y), l2 = sqrtf(e2x * e2x + e2y * e2y);
    const bool first = l1 > l2 || (l1 == l2 && fabsf(e1x) >= fabsf(e2x));
    const float lng = first ? l1 : l2, sht = first ? l2 : l1;
    float ux = 1.0f, uy = 0.0f;
    if (lng > 0.0f) ux = (first ? e1x : e2x) / lng, uy = (first ? e1y : e2y) / lng;
    if (ux < 0.0f || (ux == 0.0f && uy < 0.0f)) ux = -ux, uy = -uy;
    const float cx = 0.25f * ((a.x + a.z) + (c.x + c.z)), cy = 0.25f * ((a.y + a.w) + (c.y + c.w));
    reinterpret_cast<float4*>(frames)[2 * (long)i] = make_float4(cx, cy, ux, uy);
    reinterpret_cast<float4*>(frames)[2 * (long)i + 1] = make_float4(lng, sht, 0.0f, 0.0f);
    accept[i] = kNoAccept;
    len_sorted[i] = 0;  // a table with holes (only possible with NaN centres, whose ranks can collide) then describes empty lines, in bounds
    head_of_line[i] = -1;
}

// ---- links -----------------------------------------------------------------------------------------------------------------------
// Lane i walks every word j of [lo, hi) in index order (a tile of 256 frames per step, read from LDS at one address per step: a broadcast)
// and keeps the candidate with the smallest s; the strict `<` keeps the smallest j on a tie.  Called by all 256 lanes of a workgroup with
// the same range; a lane whose i is no word walks along for the staging and its result is not used.
struct Link {
    float s;  // distance along i's long axis to the chosen word (> 0); meaningless when j < 0
    int j;    // the chosen word, or -1
};
__device__ __forceinline__ Link nearest_follower(const float* __restrict__ frames, int lo, int hi, int i, bool is_word, float max_gap, float min_cos) {
    __shared__ float4 s_a[kTile], s_b[kTile];
    const int t = threadIdx.x;
    float4 fa = make_float4(0.0f, 0.0f, 1.0f, 0.0f), fb = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (is_word) fa = reinterpret_cast<const float4*>(frames)[2 * (long)i], fb = reinterpret_cast<const float4*>(frames)[2 * (long)i + 1];
    const float cxi = fa.x, cyi = fa.y, uxi = fa.z, uyi = fa.w, lngi = fb.x, shti = fb.y;
    const float vxi = -uyi, vyi = uxi;
    const float halfi = 0.5f * lngi;
    Link best = {0.0f, -1};
    for (int j0 = lo; j0 < hi; j0 += kTile) {
        const int m = min(kTile, hi - j0);
        __syncthreads();
        if (t < m) s_a[t] = reinterpret_cast<const float4*>(frames)[2 * (long)(j0 + t)], s_b[t] = reinterpret_cast<const float4*>(frames)[2 * (long)(j0 + t) + 1];
        __syncthreads();
#pragma unroll 4
        for (int q = 0; q < m; ++q) {
            const float4 ja = s_a[q], jb = s_b[q];
            const float dx = ja.x - cxi, dy = ja.y - cyi;
            const float s = dx * uxi + dy * uyi;
            const float tt = dx * vxi + dy * vyi;
            const float gap = (s - halfi) - 0.5f * jb.x;
            const float cs = uxi * ja.z + uyi * ja.w;
            const bool cand = s > 0.0f && fabsf(tt) <= 0.5f * fminf(shti, jb.y) && gap <= max_gap * fmaxf(shti, jb.y) && cs >= min_cos &&
                              (dx > 0.0f || (dx == 0.0f && dy > 0.0f));
            if (cand && (best.j < 0 || s < best.s)) best.s = s, best.j = j0 + q;
        }
    }
    return best;
}
// Word i records its choice, and the chosen word learns of i through atomicMin(bits(s) << 32 | i): s > 0, so its bit pattern orders as its
// value, and the low word breaks ties by the smallest chooser.
__device__ __forceinline__ void store_link(int i, Link best, int* __restrict__ chosen, unsigned long long* __restrict__ accept) {
    chosen[i] = best.j;
    if (best.j >= 0) atomicMin(&accept[best.j], ((unsigned long long)__float_as_uint(best.s) << 32) | (unsigned)i);
}
__global__ __launch_bounds__(kTile) void k_line_links(const float* __restrict__ frames, const int* __restrict__ count, long cap, float max_gap, float min_cos,
                                                      int* __restrict__ chosen, unsigned long long* __restrict__ accept) {
    const int n = word_count(count, cap);
    const int i = blockIdx.x * kTile + threadIdx.x;
    if (blockIdx.x * kTile >= n) return;  // (block-uniform)
    const Link best = nearest_follower(frames, 0, n, i, i < n, max_gap, min_cos);
    if (i < n) store_link(i, best, chosen, accept);
}

// A link i -> j exists iff i chose j and j accepted i.  Start of the pointer jumping: p = predecessor (itself for a head), d = 1 / 0.
__global__ __launch_bounds__(256) void k_line_resolve(const int* __restrict__ count, long cap, const int* __restrict__ chosen,
                                                      const unsigned long long* __restrict__ accept, int* __restrict__ next_word, int* __restrict__ p0,
                                                      int* __restrict__ d0) {
    const int n = word_count(count, cap);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = chosen[i];
    next_word[i] = (c >= 0 && (unsigned)accept[c] == (unsigned)i) ? c : -1;
    const unsigned long long a = accept[i];
    const bool has_pred = a != kNoAccept;
    p0[i] = has_pred ? (int)(unsigned)a : i;
    d0[i] = has_pred ? 1 : 0;
}

// ---- head, rank, line length -----------------------------------------------------------------------------------------------------
// Pointer jumping towards the head: d[i] += d[p[i]], p[i] = p[p[i]].  After r rounds every word within 2^r links of its head points at
// it, so ceil(log2 n) rounds finish any chain.  The last word of a line (no successor) writes the line's length at its head.
__device__ __forceinline__ void rank_finish(int i, int head, int rank, const int* __restrict__ next_word, int* __restrict__ head_o, int* __restrict__ rank_o,
                                            int* __restrict__ len_o) {
    head_o[i] = head, rank_o[i] = rank;
    if (next_word[i] < 0) len_o[head] = rank + 1;
}
__device__ __forceinline__ int jump_rounds(int n) {
    int r = 0;
    while ((1 << r) < n) ++r;
    return r;
}
__global__ __launch_bounds__(1024) void k_line_rank_lds(const int* __restrict__ count, long cap, const int* __restrict__ p0, const int* __restrict__ d0,
                                                        const int* __restrict__ next_word, int* __restrict__ head, int* __restrict__ rank, int* __restrict__ len) {
    __shared__ int s_p[2][kRankLdsMax], s_d[2][kRankLdsMax];
    const int n = min(word_count(count, cap), kRankLdsMax);
    for (int i = threadIdx.x; i < n; i += 1024) s_p[0][i] = p0[i], s_d[0][i] = d0[i];
    __syncthreads();
    int cur = 0;
    for (int r = jump_rounds(n); r > 0; --r, cur ^= 1) {
        for (int i = threadIdx.x; i < n; i += 1024) {
            const int q = s_p[cur][i];
            s_d[cur ^ 1][i] = s_d[cur][i] + s_d[cur][q];
            s_p[cur ^ 1][i] = s_p[cur][q];
        }
        __syncthreads();
    }
    for (int i = threadIdx.x; i < n; i += 1024) rank_finish(i, s_p[cur][i], s_d[cur][i], next_word, head, rank, len);
}
__global__ __launch_bounds__(256) void k_line_jump(const int* __restrict__ count, long cap, const int* __restrict__ pin, const int* __restrict__ din,
                                                   int* __restrict__ pout, int* __restrict__ dout) {
    const int n = word_count(count, cap);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int q = pin[i];
    dout[i] = din[i] + din[q];
    pout[i] = pin[q];
}
__global__ __launch_bounds__(256) void k_line_rank_finish(const int* __restrict__ count, long cap, const int* __restrict__ p, const int* __restrict__ d,
                                                          const int* __restrict__ next_word, int* __restrict__ head, int* __restrict__ rank, int* __restrict__ len) {
    const int n = word_count(count, cap);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) rank_finish(i, p[i], d[i], next_word, head, rank, len);
}

// ---- order -----------------------------------------------------------------------------------------------------------------------
// The line of head i is the number of heads that sort before it under (c.y, c.x, word index): a strict total order on finite centres, so the
// indices are 0..L-1 without gaps.  Same staging as k_line_links; a word that is no head is staged with a flag and counts for nothing.
__global__ __launch_bounds__(kTile) void k_line_order(const float* __restrict__ frames, const int* __restrict__ count, long cap, const int* __restrict__ head,
                                                      const int* __restrict__ len, int* __restrict__ line_idx, int* __restrict__ len_sorted,
                                                      int* __restrict__ head_of_line) {
    __shared__ float s_cy[kTile], s_cx[kTile];
    __shared__ int s_is_head[kTile];
    const int n = word_count(count, cap);
    const int t = threadIdx.x, i = blockIdx.x * kTile + t;
    if (blockIdx.x * kTile >= n) return;
    const bool mine = i < n && head[i] == i;
    float cxi = 0.0f, cyi = 0.0f;
    if (i < n) cxi = frames[8 * (long)i], cyi = frames[8 * (long)i + 1];
    int before = 0;
    for (int j0 = 0; j0 < n; j0 += kTile) {
        const int m = min(kTile, n - j0);
        __syncthreads();
        if (t < m) {
            const float2 c = *reinterpret_cast<const float2*>(frames + 8 * (long)(j0 + t));
            s_cx[t] = c.x, s_cy[t] = c.y, s_is_head[t] = head[j0 + t] == j0 + t;
        }
        __syncthreads();
#pragma unroll 4
        for (int q = 0; q < m; ++q) {
            const float cy = s_cy[q], cx = s_cx[q];
            const bool less = cy < cyi || (cy == cyi && (cx < cxi || (cx == cxi && j0 + q < i)));
            before += (s_is_head[q] && less) ? 1 : 0;
        }
    }
    if (mine) {  // before < number of heads <= n
        line_idx[i] = before;
        len_sorted[before] = len[i];
        head_of_line[before] = i;
    }
}

// One workgroup: L = number of heads, then line_offsets[0..L] = exclusive scan of the line lengths in line order, 256 at a time.
__global__ __launch_bounds__(256) void k_line_scan(const int* __restrict__ count, long cap, const int* __restrict__ head, const int* __restrict__ len_sorted,
                                                   int* __restrict__ line_offsets, int* __restrict__ n_lines) {
    __shared__ int s_total;
    const int n = word_count(count, cap);
    const int t = threadIdx.x;
    if (t == 0) s_total = 0;
    __syncthreads();
    int heads = 0;
    for (int i = t; i < n; i += 256) heads += head[i] == i;
    atomicAdd(&s_total, heads);  // (integer: the sum does not depend on the order)
    __syncthreads();
    const int L = s_total;
    int base = 0;
    for (int l0 = 0; l0 < L; l0 += 256) {
        const int l = l0 + t;
        const int v = l < L ? len_sorted[l] : 0;
        const int2 sc = block_scan_256(v);
        if (l < L) line_offsets[l] = base + sc.x - v;
        base += sc.y;
    }
    if (t == 0) line_offsets[L] = base, *n_lines = L;
}

__global__ __launch_bounds__(256) void k_line_scatter(const int* __restrict__ count, long cap, const int* __restrict__ head, const int* __restrict__ rank,
                                                      const int* __restrict__ line_idx, const int* __restrict__ line_offsets, int* __restrict__ line_of_word,
                                                      int* __restrict__ word_order) {
    const int n = word_count(count, cap);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int l = line_idx[head[i]];
    line_of_word[i] = l;
    const long pos = (long)line_offsets[l] + rank[i];
    if (pos >= 0 && pos < n) word_order[pos] = i;  // (always, on finite input)
}

// ---- line quads ------------------------------------------------------------------------------------------------------------------
// One wave per line.  u_L = normalise(sum of lng_i * u_i), added one word after the other in chain order (lane k of a chunk holds word k's
// term; the running sum takes them by lane index, so every lane holds the same bits).  Then each lane projects the corners of its words and
// the extrema meet in a butterfly of min / max, which no order of evaluation changes.  A one-word line is that word's quad, copied.
__global__ __launch_bounds__(256) void k_line_quads(const float* __restrict__ quads, const float* __restrict__ frames, const int* __restrict__ count, long cap,
                                                    const int* __restrict__ n_lines, const int* __restrict__ line_offsets, const int* __restrict__ word_order,
                                                    float* __restrict__ line_quads) {
    const int n = word_count(count, cap);
    const int lane = threadIdx.x & 63;
    const int l = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (l >= min(*n_lines, n)) return;  // rows from L on are left untouched
    const int off = min(max(line_offsets[l], 0), n);
    const int cnt = min(max(line_offsets[l + 1] - off, 0), n - off);
    if (cnt == 0) return;
    if (cnt == 1) {
        const int w = word_order[off];
        if (lane < 2 && (unsigned)w < (unsigned)n) reinterpret_cast<float4*>(line_quads)[2 * (long)l + lane] = reinterpret_cast<const float4*>(quads)[2 * (long)w + lane];
        return;
    }
    float sx = 0.0f, sy = 0.0f;
    for (int k0 = 0; k0 < cnt; k0 += 64) {
        float wx = 0.0f, wy = 0.0f;
        if (k0 + lane < cnt) {
            const int w = word_order[off + k0 + lane];
            if ((unsigned)w < (unsigned)n) {
                const float4 fa = reinterpret_cast<const float4*>(frames)[2 * (long)w];
                const float lng = frames[8 * (long)w + 4];
                wx = lng * fa.z, wy = lng * fa.w;
            }
        }
        const int m = min(64, cnt - k0);
        for (int q = 0; q < m; ++q) sx = sx + __shfl(wx, q, 64), sy = sy + __shfl(wy, q, 64);
    }
    const float norm = sqrtf(sx * sx + sy * sy);
    float ux = 1.0f, uy = 0.0f;
    if (norm > 0.0f) ux = sx / norm, uy = sy / norm;
    const float vx = -uy, vy = ux;
    float lo_u = INFINITY, hi_u = -INFINITY, lo_v = INFINITY, hi_v = -INFINITY;
    for (int k = lane; k < cnt; k += 64) {
        const int w = word_order[off + k];
        if ((unsigned)w >= (unsigned)n) continue;
        const float4 a = reinterpret_cast<const float4*>(quads)[2 * (long)w], c = reinterpret_cast<const float4*>(quads)[2 * (long)w + 1];
        const float xs[4] = {a.x, a.z, c.x, c.z}, ys[4] = {a.y, a.w, c.y, c.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float pu = xs[q] * ux + ys[q] * uy, pv = xs[q] * vx + ys[q] * vy;
            lo_u = fminf(lo_u, pu), hi_u = fmaxf(hi_u, pu), lo_v = fminf(lo_v, pv), hi_v = fmaxf(hi_v, pv);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo_u = fminf(lo_u, __shfl_xor(lo_u, o, 64)), hi_u = fmaxf(hi_u, __shfl_xor(hi_u, o, 64));
        lo_v = fminf(lo_v, __shfl_xor(lo_v, o, 64)), hi_v = fmaxf(hi_v, __shfl_xor(hi_v, o, 64));
    }
    if (lane == 0) {
        reinterpret_cast<float4*>(line_quads)[2 * (long)l] = make_float4(lo_u * ux + lo_v * vx, lo_u * uy + lo_v * vy, hi_u * ux + lo_v * vx, hi_u * uy + lo_v * vy);
        reinterpret_cast<float4*>(line_quads)[2 * (long)l + 1] = make_float4(hi_u * ux + hi_v * vx, hi_u * uy + hi_v * vy, lo_u * ux + hi_v * vx, lo_u * uy + hi_v * vy);
    }
}

// ---- page batches ------------------------------------------------------------------------------------------------------------------
struct PagesWs {
    int *blk_offs;  // [B + 1] first workgroup of every page
    int *heads;     // [B] heads (= lines) per page
};
inline PagesWs ws_split_pages(void* ws, long cap, int B) {
    PagesWs w;
    char* p = static_cast<char*>(ws) + ws_cap(cap) * kWsBytesPerWord;
    w.blk_offs = reinterpret_cast<int*>(p), p += ws_cap(B + 1) * 4;
    w.heads = reinterpret_cast<int*>(p);
    return w;
}

// word range of page p, clamped so that offsets that are not an ascending scan still index inside the n words
__device__ __forceinline__ int2 page_range(const int* __restrict__ word_offs, int p, int n) {
    const int lo = min(max(word_offs[p], 0), n);
    return make_int2(lo, min(max(word_offs[p + 1], lo), n));
}
// the last p in [0, B) with offs[p] <= k, for an ascending offs with offs[0] <= k: the page of workgroup k in blk_offs (k < blk_offs[B]; pages
// without words own no workgroup and are passed over) and the page of word k in word_offs
__device__ __forceinline__ int last_le(const int* __restrict__ offs, int B, int k) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (offs[mid] <= k) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_pages_init(const int* __restrict__ count, long cap, int B, int* __restrict__ chosen, int* __restrict__ line_idx,
                                                    int* __restrict__ heads) {
    const int n = word_count(count, cap);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) chosen[i] = -1, line_idx[i] = 0;
    if (i < B) heads[i] = 0;
}

// One workgroup: out[0..B] = exclusive scan over the pages, 256 at a time, of ceil(n_p / per) (per > 0, from word_offs) or of vals[p] (per == 0).
__global__ __launch_bounds__(256) void k_page_scan(const int* __restrict__ word_offs, const int* __restrict__ vals, const int* __restrict__ count, long cap, int B,
                                                   int per, int* __restrict__ out) {
    const int n = word_count(count, cap);
    const int t = threadIdx.x;
    int base = 0;
    for (int p0 = 0; p0 < B; p0 += 256) {
        const int p = p0 + t;
        int v = 0;
        if (p < B) {
            if (per > 0) {
                const int2 r = page_range(word_offs, p, n);
                v = (r.y - r.x + per - 1) / per;
            } else {
                v = min(max(vals[p], 0), n);
            }
        }
        const int2 sc = block_scan_256(v);
        if (p < B) out[p] = base + sc.x - v;
        base += sc.y;
    }
    if (t == 0) out[B] = base;
}

// k_line_links with one page per workgroup: the walk covers word_offs[p] .. word_offs[p + 1] only, so a word of another page is never a
// candidate and the work is the sum of n_p^2.
__global__ __launch_bounds__(kTile) void k_line_links_pages(const float* __restrict__ frames, const int* __restrict__ word_offs, const int* __restrict__ blk_offs, int B,
                                                            const int* __restrict__ count, long cap, float max_gap, float min_cos, int* __restrict__ chosen,
                                                            unsigned long long* __restrict__ accept) {
    const int n = word_count(count, cap);
    const int k = blockIdx.x;
    if (k >= blk_offs[B]) return;  // (block-uniform)
    const int p = last_le(blk_offs, B, k);
    const int2 r = page_range(word_offs, p, n);
    const int i = r.x + (k - blk_offs[p]) * kTile + threadIdx.x;
    const Link best = nearest_follower(frames, r.x, r.y, i, i < r.y, max_gap, min_cos);
    if (i < r.y) store_link(i, best, chosen, accept);
}

// k_line_order per page: the rank of head i among the heads of its own page under (c.y, c.x, word index), left in line_idx[i] for
// k_line_place_pages; the heads of each page are counted with an integer atomic.  The count is k_line_order's text over the page's range: as
// one inlined function hipcc vectorises the loop differently and the order stage runs 8 to 15 % slower, so the two stay separate texts.
__global__ __launch_bounds__(kTile) void k_line_order_pages(const float* __restrict__ frames, const int* __restrict__ word_offs, const int* __restrict__ blk_offs, int B,
                                                            const int* __restrict__ count, long cap, const int* __restrict__ head, int* __restrict__ line_idx,
                                                            int* __restrict__ heads) {
    __shared__ float s_cy[kTile], s_cx[kTile];
    __shared__ int s_is_head[kTile];
    const int n = word_count(count, cap);
    const int k = blockIdx.x;
    if (k >= blk_offs[B]) return;
    const int p = last_le(blk_offs, B, k);
    const int2 r = page_range(word_offs, p, n);
    const int t = threadIdx.x, i = r.x + (k - blk_offs[p]) * kTile + t;
    const bool mine = i < r.y && head[i] == i;
    float cxi = 0.0f, cyi = 0.0f;
    if (i < r.y) cxi = frames[8 * (long)i], cyi = frames[8 * (long)i + 1];
    int before = 0;
    for (int j0 = r.x; j0 < r.y; j0 += kTile) {
        const int m = min(kTile, r.y - j0);
        __syncthreads();
        if (t < m) {
            const float2 c = *reinterpret_cast<const float2*>(frames + 8 * (long)(j0 + t));
            s_cx[t] = c.x, s_cy[t] = c.y, s_is_head[t] = head[j0 + t] == j0 + t;
        }
        __syncthreads();
#pragma unroll 4
        for (int q = 0; q < m; ++q) {
            const float cy = s_cy[q], cx = s_cx[q];
            const bool less = cy < cyi || (cy == cyi && (cx < cxi || (cx == cxi && j0 + q < i)));
            before += (s_is_head[q] && less) ? 1 : 0;
        }
    }
    if (mine) {
        line_idx[i] = before;
        atomicAdd(&heads[p], 1);  // (integer: the sum does not depend on the order)
    }
}

__global__ __launch_bounds__(256) void k_line_place_pages(const int* __restrict__ word_offs, int B, const int* __restrict__ count, long cap, const int* __restrict__ head,
                                                          const int* __restrict__ len, const int* __restrict__ line_page_offs, int* __restrict__ line_idx,
                                                          int* __restrict__ len_sorted, int* __restrict__ head_of_line, int* __restrict__ page_of_line) {
    const int n = word_count(count, cap);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || head[i] != i) return;
    const int p = last_le(word_offs, B, i);
    const int l = line_page_offs[p] + line_idx[i];
    if ((unsigned)l >= (unsigned)n) {  // (never, on finite input with ascending offsets)
        line_idx[i] = 0;
        return;
    }
    line_idx[i] = l;
    len_sorted[l] = len[i];
    head_of_line[l] = i;
    page_of_line[l] = p;
}

inline unsigned blocks(long n, int per) { return (unsigned)((n + per - 1) / per); }
constexpr long kMaxWords = 1L << 24;
constexpr int kMaxPages = 1 << 20;

}  // namespace

extern "C" {

long ocrs_text_lines_ws_bytes(long cap) { return cap > 0 && cap <= kMaxWords ? ws_cap(cap) * kWsBytesPerWord : 0; }

int ocrs_line_links(const float* quads, const int* count, long cap, float max_gap, float min_cos, int* next_word, void* ws, long ws_bytes, hipStream_t st) {
    OCRS_CHECK_ARG(cap >= 0 && cap <= kMaxWords);
    if (cap == 0) return OCRS_OK;
    OCRS_CHECK_ARG(quads && next_word && ws && aligned16(quads) && aligned16(ws) && ws_bytes >= ocrs_text_lines_ws_bytes(cap));
    const LinesWs w = ws_split(ws, cap);
    hipLaunchKernelGGL(k_line_frames, dim3(blocks(cap, 256)), dim3(256), 0, st, quads, count, cap, w.frames, w.accept, w.len_sorted, w.head_of_line);
    hipLaunchKernelGGL(k_line_links, dim3(blocks(cap, kTile)), dim3(kTile), 0, st, (const float*)w.frames, count, cap, max_gap, min_cos, w.chosen, w.accept);
    hipLaunchKernelGGL(k_line_resolve, dim3(blocks(cap, 256)), dim3(256), 0, st, count, cap, (const int*)w.chosen, (const unsigned long long*)w.accept, next_word,
                       w.pa, w.da);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

int ocrs_line_rank(const int* count, long cap, const int* next_word, void* ws, long ws_bytes, hipStream_t st) {
    OCRS_CHECK_ARG(cap >= 0 && cap <= kMaxWords);
    if (cap == 0) return OCRS_OK;
    OCRS_CHECK_ARG(next_word && ws && aligned16(ws) && ws_bytes >= ocrs_text_lines_ws_bytes(cap));
    const LinesWs w = ws_split(ws, cap);
    if (cap <= kRankLdsMax) {
        hipLaunchKernelGGL(k_line_rank_lds, dim3(1), dim3(1024), 0, st, count, cap, (const int*)w.pa, (const int*)w.da, next_word, w.head, w.rank, w.len);
    } else {
        int *pin = w.pa, *din = w.da, *pout = w.pb, *dout = w.db;
        for (long reach = 1; reach < cap; reach <<= 1) {
            hipLaunchKernelGGL(k_line_jump, dim3(blocks(cap, 256)), dim3(256), 0, st, count, cap, (const int*)pin, (const int*)din, pout, dout);
            int* tp = pin;
            pin = pout, pout = tp;
            tp = din, din = dout, dout = tp;
        }
        hipLaunchKernelGGL(k_line_rank_finish, dim3(blocks(cap, 256)), dim3(256), 0, st, count, cap, (const int*)pin, (const int*)din, next_word, w.head, w.rank,
                           w.len);
    }
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

int ocrs_line_order(const int* count, long cap, int* n_lines, int* line_of_word, int* word_order, int* line_offsets, void* ws, long ws_bytes, hipStream_t st) {
    OCRS_CHECK_ARG(cap >= 0 && cap <= kMaxWords);
    if (cap == 0) return OCRS_OK;
    OCRS_CHECK_ARG(n_lines && line_offsets && line_of_word && word_order && ws && aligned16(ws) && ws_bytes >= ocrs_text_lines_ws_bytes(cap));
    const LinesWs w = ws_split(ws, cap);
    hipLaunchKernelGGL(k_line_order, dim3(blocks(cap, kTile)), dim3(kTile), 0, st, (const float*)w.frames, count, cap, (const int*)w.head, (const int*)w.len,
                       w.line_idx, w.len_sorted, w.head_of_line);
    hipLaunchKernelGGL(k_line_scan, dim3(1), dim3(256), 0, st, count, cap, (const int*)w.head, (const int*)w.len_sorted, line_offsets, n_lines);
    hipLaunchKernelGGL(k_line_scatter, dim3(blocks(cap, 256)), dim3(256), 0, st, count, cap, (const int*)w.head, (const int*)w.rank, (const int*)w.line_idx,
                       (const int*)line_offsets, line_of_word, word_order);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

int ocrs_line_quads(const float* quads, const int* count, long cap, const int* n_lines, const int* line_offsets, const int* word_order, float* line_quads,
                    void* ws, long ws_bytes, hipStream_t st) {
    OCRS_CHECK_ARG(cap >= 0 && cap <= kMaxWords);
    if (cap == 0) return OCRS_OK;
    OCRS_CHECK_ARG(quads && n_lines && line_offsets && word_order && line_quads && ws && aligned16(quads) && aligned16(line_quads) && aligned16(ws) &&
                   ws_bytes >= ocrs_text_lines_ws_bytes(cap));
    const LinesWs w = ws_split(ws, cap);
    hipLaunchKernelGGL(k_line_quads, dim3(blocks(cap, 4)), dim3(256), 0, st, quads, (const float*)w.frames, count, cap, n_lines, line_offsets, word_order,
                       line_quads);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

// ---- page batches: the total word_offs[B] is the device count of the unchanged kernels ----------------------------------------------
long ocrs_text_lines_pages_ws_bytes(long cap, int B) {
    return cap > 0 && cap <= kMaxWords && B > 0 && B <= kMaxPages ? ws_cap(cap) * kWsBytesPerWord + 2 * ws_cap(B + 1) * 4 : 0;
}

int ocrs_line_links_pages(const float* quads, const int* word_offs, int B, long cap, float max_gap, float min_cos, int* next_word, void* ws, long ws_bytes,
                          hipStream_t st) {
    OCRS_CHECK_ARG(cap >= 0 && cap <= kMaxWords && B >= 0 && B <= kMaxPages);
    if (cap == 0 || B == 0) return OCRS_OK;
    OCRS_CHECK_ARG(quads && word_offs && next_word && ws && aligned16(quads) && aligned16(ws) && ws_bytes >= ocrs_text_lines_pages_ws_bytes(cap, B));
    const LinesWs w = ws_split(ws, cap);
    const PagesWs pw = ws_split_pages(ws, cap, B);
    const int* count = word_offs + B;
    const unsigned page_blocks = blocks(cap, kTile) + (unsigned)B;  // >= the sum of ceil(n_p / kTile)
    hipLaunchKernelGGL(k_line_frames, dim3(blocks(cap, 256)), dim3(256), 0, st, quads, count, cap, w.frames, w.accept, w.len_sorted, w.head_of_line);
    hipLaunchKernelGGL(k_pages_init, dim3(blocks(cap > B ? cap : B, 256)), dim3(256), 0, st, count, cap, B, w.chosen, w.line_idx, pw.heads);
    hipLaunchKernelGGL(k_page_scan, dim3(1), dim3(256), 0, st, word_offs, (const int*)nullptr, count, cap, B, kTile, pw.blk_offs);
    hipLaunchKernelGGL(k_line_links_pages, dim3(page_blocks), dim3(kTile), 0, st, (const float*)w.frames, word_offs, (const int*)pw.blk_offs, B, count, cap, max_gap,
                       min_cos, w.chosen, w.accept);
    hipLaunchKernelGGL(k_line_resolve, dim3(blocks(cap, 256)), dim3(256), 0, st, count, cap, (const int*)w.chosen, (const unsigned long long*)w.accept, next_word,
                       w.pa, w.da);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

int ocrs_line_rank_pages(const int* word_offs, int B, long cap, const int* next_word, void* ws, long ws_bytes, hipStream_t st) {
    OCRS_CHECK_ARG(cap >= 0 && cap <= kMaxWords && B >= 0 && B <= kMaxPages);
    if (cap == 0 || B == 0) return OCRS_OK;
    OCRS_CHECK_ARG(word_offs && ws_bytes >= ocrs_text_lines_pages_ws_bytes(cap, B));
    return ocrs_line_rank(word_offs + B, cap, next_word, ws, ws_bytes, st);  // links never leave a page: the chains are the flat array's
}

int ocrs_line_order_pages(const int* word_offs, int B, long cap, int* n_lines, int* line_of_word, int* word_order, int* line_offsets, int* line_page_offs,
                          int* page_of_line, void* ws, long ws_bytes, hipStream_t st) {
    OCRS_CHECK_ARG(cap >= 0 && cap <= kMaxWords && B >= 0 && B <= kMaxPages);
    if (cap == 0 || B == 0) return OCRS_OK;
    OCRS_CHECK_ARG(word_offs && n_lines && line_offsets && line_of_word && word_order && line_page_offs && page_of_line && ws && aligned16(ws) &&
                   ws_bytes >= ocrs_text_lines_pages_ws_bytes(cap, B));
    const LinesWs w = ws_split(ws, cap);
    const PagesWs pw = ws_split_pages(ws, cap, B);
    const int* count = word_offs + B;
    hipLaunchKernelGGL(k_line_order_pages, dim3(blocks(cap, kTile) + (unsigned)B), dim3(kTile), 0, st, (const float*)w.frames, word_offs, (const int*)pw.blk_offs, B,
                       count, cap, (const int*)w.head, w.line_idx, pw.heads);
    hipLaunchKernelGGL(k_page_scan, dim3(1), dim3(256), 0, st, word_offs, (const int*)pw.heads, count, cap, B, 0, line_page_offs);
    hipLaunchKernelGGL(k_line_place_pages, dim3(blocks(cap, 256)), dim3(256), 0, st, word_offs, B, count, cap, (const int*)w.head, (const int*)w.len,
                       (const int*)line_page_offs, w.line_idx, w.len_sorted, w.head_of_line, page_of_line);
    hipLaunchKernelGGL(k_line_scan, dim3(1), dim3(256), 0, st, count, cap, (const int*)w.head, (const int*)w.len_sorted, line_offsets, n_lines);
    hipLaunchKernelGGL(k_line_scatter, dim3(blocks(cap, 256)), dim3(256), 0, st, count, cap, (const int*)w.head, (const int*)w.rank, (const int*)w.line_idx,
                       (const int*)line_offsets, line_of_word, word_order);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

int ocrs_line_quads_pages(const float* quads, const int* word_offs, int B, long cap, const int* n_lines, const int* line_offsets, const int* word_order,
                          float* line_quads, void* ws, long ws_bytes, hipStream_t st) {
    OCRS_CHECK_ARG(cap >= 0 && cap <= kMaxWords && B >= 0 && B <= kMaxPages);
    if (cap == 0 || B == 0) return OCRS_OK;
    OCRS_CHECK_ARG(word_offs && ws_bytes >= ocrs_text_lines_pages_ws_bytes(cap, B));
    return ocrs_line_quads(quads, word_offs + B, cap, n_lines, line_offsets, word_order, line_quads, ws, ws_bytes, st);  // a line's words are one page's
}

}  // extern "C"
