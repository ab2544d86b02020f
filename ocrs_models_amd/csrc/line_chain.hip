// Chain crops (DESIGN.md §21 states the rule; the numpy restatement is tests/chain_ref.py; Python: inference/chain.py): a line's crop is cut
// along the polyline of its words -- the spine -- at one constant height, so every word of a curved line sits upright and at full height
// in the crop.  Runs between the line stage and the recogniser in the place of the line quad's rectangle; every count stays on the device.
//
//   k_line_spines          one wave per line, 64 words per round: each lane its word's frame (crop_frame.h), knots and the gap behind it; the
//                          segments' starts are one running sum taken in lane (chain) order -> spine [2N][8], line_dims [N][2] = S, H
//   (crop plan)            k_crop_plan<DimsSize> of ocr_infer.hip: the plan of ocrs_crop_plan with (h, w) from (H, S)
//   k_rectify_chain        the tiling of k_rectify_crops (crop_sample.h: kTileElems, crop_of_tile, sample_u8); what is new per lane is
//   k_rectify_chain_pages  finding the segment of each of its 4 samples (line_chain.h), in LDS where the line's rows fit kSpineLdsRows
//   k_char_boxes_chain     DESIGN.md §17 (b) through the spine: a character's quad is P(s0, -H/2), P(s1, -H/2), P(s1, +H/2), P(s0, +H/2)
//   k_word_chars_chain     §17 (c) with the boundaries b_j = start(word j + 1) - 0.5 len(gap j), read off the spine table
//
// The word frame is crop_frame()'s, compiled as it is everywhere else; everything this file adds to it -- knots, gaps, starts, sample
// positions -- is fp32 with one rounding per operation (no fused multiply-add), so the restatement follows it operation by operation.  No
// atomics, nothing synchronises: equal input gives equal bytes.
#include "char_range.h"
#include "crop_frame.h"
#include "crop_sample.h"
#include "line_chain.h"  // (fp contract off from here on)

namespace {

// Rows of one line that a sampler workgroup stages in LDS: 256 rows of 32 bytes = 8 KB, two 16-byte loads per lane.  A line of up to 128
// words fits; 8 KB leaves the workgroups per CU bounded by waves (8 x 4 waves of the CU's 32), not by LDS (160 KB / 8 KB = 20).
constexpr int kSpineLdsRows = 256;

__device__ __forceinline__ long line_count(const int* __restrict__ n_lines, long cap) { return min((long)max(*n_lines, 0), cap); }

// words off .. off + n - 1 of word_order are line l's, n >= 1, all inside the wcap words: false for a line table that does not say so
__device__ __forceinline__ bool line_range(const int* __restrict__ line_offsets, long l, long wcap, int& off, int& n) {
    off = line_offsets[l], n = line_offsets[l + 1] - off;
    return off >= 0 && n > 0 && (long)off + n <= wcap;
}

// ---- spines ------------------------------------------------------------------------------------------------------------------------
struct Knots {
    float lx, ly, rx, ry, ux, uy, lng, sht;  // L, R: mid-points of the word's left and right edges
};
__device__ __forceinline__ Knots word_knots(const float* __restrict__ words, long wcap, long w) {
    Knots k = {0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f};  // (a word index outside the words: a point at the origin)
    if (w < 0 || w >= wcap) return k;
    const CropFrame f = crop_frame(words + w * 8);
    const float hs = 0.5f * f.sht, vx = -f.uy, vy = f.ux;
    k.lx = f.ox + hs * vx, k.ly = f.oy + hs * vy;
    k.rx = k.lx + f.lng * f.ux, k.ry = k.ly + f.lng * f.uy;
    k.ux = f.ux, k.uy = f.uy, k.lng = f.lng, k.sht = f.sht;
    return k;
}

// One wave per line (four lines per workgroup); lane k of a round holds word base + k of the chain: its knots, and from the next word's the
// gap behind it.  The starts are ONE running sum over word, gap, word, gap ... in chain order: every lane adds the same terms in the same
// order (broadcast by lane index), so all hold the same bits, and the lane whose turn it is keeps the sum before its word and before its gap.
// The sum and the running maximum of the heights are carried from round to round.
__global__ __launch_bounds__(256) void k_line_spines(const float* __restrict__ words, long wcap, const int* __restrict__ n_lines, long cap,
                                                     const int* __restrict__ line_offsets, const int* __restrict__ word_order, float* __restrict__ spine,
                                                     float* __restrict__ line_dims) {
    const int lane = threadIdx.x & 63;
    const long l = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (l >= line_count(n_lines, cap)) return;  // (wave-uniform; the kernel has no barrier) rows from n_lines on are left untouched
    int off, n;
    if (!line_range(line_offsets, l, wcap, off, n)) return;
    float run = 0.0f, hmax = 0.0f;
    for (int base = 0; base < n; base += 64) {
        const int k = base + lane;
        const bool live = k < n;
        Knots a = {0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f};
        float gap = 0.0f, dx = 0.0f, dy = 0.0f;
        if (live) a = word_knots(words, wcap, word_order[off + k]);
        if (live && k + 1 < n) {
            const Knots b = word_knots(words, wcap, word_order[off + k + 1]);
            const float ex = b.lx - a.rx, ey = b.ly - a.ry;
            const float g = sqrtf(ex * ex + ey * ey);
            if (g > 0.0f && ex * (a.ux + b.ux) + ey * (a.uy + b.uy) > 0.0f) gap = g, dx = ex / g, dy = ey / g;  // else the spine jumps from R to L
        }
        float start_w = 0.0f, start_g = 0.0f;
        const int m = min(64, n - base);
        for (int q = 0; q < m; ++q) {
            const float lw = __shfl(a.lng, q, 64), lg = __shfl(gap, q, 64);
            if (lane == q) start_w = run;
            run = run + lw;
            if (lane == q) start_g = run;
            run = run + lg;
        }
        hmax = fmaxf(hmax, a.sht);
        if (live) {
            float4* row = reinterpret_cast<float4*>(spine) + 4 * ((long)off + k);
            row[0] = make_float4(start_w, a.lng, a.lx, a.ly);
            row[1] = make_float4(a.ux, a.uy, 0.0f, 0.0f);
            const bool last = k == n - 1;  // no gap behind the last word: an all-zero row
            row[2] = last ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : make_float4(start_g, gap, a.rx, a.ry);
            row[3] = last ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : make_float4(dx, dy, 0.0f, 0.0f);
        }
    }
    hmax = wave_max(hmax);
    if (lane == 0) reinterpret_cast<float2*>(line_dims)[l] = make_float2(run, hmax);
}

// ---- the sampler ---------------------------------------------------------------------------------------------------------------------
// This lane's 4 samples of its tile: e0 is the first one's element in the (h, w) crop of hw elements.
__device__ __forceinline__ float4 chain_samples(const uint8_t* __restrict__ page, int H, int W, const float4* __restrict__ rows, int nseg, float S, float Hl, int h, int w,
                                                long e0, long hw) {
    int y = (int)(e0 / w), x = (int)(e0 - (long)y * w);
    float s[4], t[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        s[k] = ((float)x + 0.5f) / (float)w * S;
        t[k] = (((float)y + 0.5f) / (float)h - 0.5f) * Hl;
        if (++x == w) x = 0, ++y;
    }
    int seg[4];
    spine_segments<4>(rows, nseg, s, seg);  // the four samples may lie on different segments, and on different rows of the crop
    float out[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        out[k] = 0.0f;
        if (e0 + k < hw) {
            const float2 p = spine_point(rows, seg[k], s[k], t[k]);
            out[k] = sample_u8(page, H, W, p.x, p.y);
        }
    }
    return make_float4(out[0], out[1], out[2], out[3]);
}

// One workgroup = tile `tile` of crop (= line) `crop`, as rectify_tile of ocr_infer.hip.  The line's 2 n - 1 segment rows are staged in LDS
// with 16-byte loads where they fit, and the lanes bisect there; a longer line is bisected in global memory (its rows are L2-resident: the
// tiles of one crop run next to each other).  All branches up to the barrier are workgroup-uniform.
__device__ __forceinline__ void rectify_chain_tile(const uint8_t* __restrict__ page, int H, int W, const float* __restrict__ spine, const float* __restrict__ line_dims,
                                                   const int* __restrict__ line_offsets, long wcap, const int* __restrict__ plan, long crop, long long tile,
                                                   float* __restrict__ packed, long packed_floats) {
    __shared__ float4 s_rows[2 * kSpineLdsRows];
    int off, n;
    if (!line_range(line_offsets, crop, wcap, off, n)) return;
    const int nseg = 2 * n - 1;
    const float4* rows = reinterpret_cast<const float4*>(spine) + 4 * (long)off;
    const float2 dims = reinterpret_cast<const float2*>(line_dims)[crop];  // S, H
    const int4 pl = *reinterpret_cast<const int4*>(plan + crop * 8);       // h, w, ow, packed offset
    const int h = pl.x, w = pl.y;
    const long hw = (long)h * w;
    const long e0 = (long)(tile - plan[crop * 8 + 5]) * kTileElems + threadIdx.x * 4;
    const bool mine = h > 0 && w > 0 && e0 < hw && (long)pl.w + e0 + 4 <= packed_floats;
    float4 out;
    if (nseg <= kSpineLdsRows) {
        for (int i = threadIdx.x; i < 2 * nseg; i += 256) s_rows[i] = rows[i];
        __syncthreads();
        if (!mine) return;
        out = chain_samples(page, H, W, s_rows, nseg, dims.x, dims.y, h, w, e0, hw);
    } else {
        if (!mine) return;
        out = chain_samples(page, H, W, rows, nseg, dims.x, dims.y, h, w, e0, hw);
    }
    *reinterpret_cast<float4*>(packed + pl.w + e0) = out;
}

__global__ __launch_bounds__(256) void k_rectify_chain(const uint8_t* __restrict__ page, int H, int W, const float* __restrict__ spine,
                                                       const float* __restrict__ line_dims, const int* __restrict__ line_offsets, long wcap,
                                                       const int* __restrict__ plan, const long long* __restrict__ totals, float* __restrict__ packed,
                                                       long packed_floats) {
    const long long tile = blockIdx.x;
    const long n = (long)totals[0];
    if (n <= 0 || tile >= totals[3]) return;
    rectify_chain_tile(page, H, W, spine, line_dims, line_offsets, wcap, plan, crop_of_tile(plan, n, tile), tile, packed, packed_floats);
}

// The same from a store of pages, as k_rectify_crops_pages: the line's page is looked up once per workgroup.
__global__ __launch_bounds__(256) void k_rectify_chain_pages(const uint8_t* __restrict__ pages, long pages_bytes, const long long* __restrict__ page_offs,
                                                             const int* __restrict__ page_sizes, int B, const float* __restrict__ spine,
                                                             const float* __restrict__ line_dims, const int* __restrict__ line_offsets, long wcap,
                                                             const int* __restrict__ page_of_line, const int* __restrict__ plan,
                                                             const long long* __restrict__ totals, float* __restrict__ packed, long packed_floats) {
    const long long tile = blockIdx.x;
    const long n = (long)totals[0];
    if (n <= 0 || tile >= totals[3]) return;
    const long crop = crop_of_tile(plan, n, tile);
    const int pg = page_of_line[crop];
    if ((unsigned)pg >= (unsigned)B) return;
    const int H = page_sizes[2 * pg], W = page_sizes[2 * pg + 1];
    const long long poff = page_offs[pg];
    if (H <= 0 || W <= 0 || poff < 0 || poff + (long long)H * W > pages_bytes) return;  // a page that is not inside the store is not read
    rectify_chain_tile(pages + poff, H, W, spine, line_dims, line_offsets, wcap, plan, crop, tile, packed, packed_floats);
}

// ---- characters ----------------------------------------------------------------------------------------------------------------------
// One workgroup per row p of the span arrays, the crop of line i = plan[p][7]; one lane = one character: two 16-byte stores for its quad.
__global__ __launch_bounds__(64) void k_char_boxes_chain(const float* __restrict__ spine, const float* __restrict__ line_dims, const int* __restrict__ line_offsets,
                                                         long wcap, const int* __restrict__ plan, long cap, int ld, const int* __restrict__ lens,
                                                         const int* __restrict__ t0, const int* __restrict__ t1, float* __restrict__ s0, float* __restrict__ s1,
                                                         float* __restrict__ cquads) {
    const long p = blockIdx.x;
    const long i = plan[p * 8 + 7];
    if (i < 0 || i >= cap) return;
    const int len = min(max(lens[p], 0), ld);
    int off, n;
    if (len == 0 || !line_range(line_offsets, i, wcap, off, n)) return;
    const int nseg = 2 * n - 1;
    const float4* rows = reinterpret_cast<const float4*>(spine) + 4 * (long)off;
    const float2 dims = reinterpret_cast<const float2*>(line_dims)[i];  // S, H
    const int ow = max(plan[i * 8 + 2], 1);
    const float hh = 0.5f * dims.y;
    for (int k = threadIdx.x; k < len; k += 64) {
        const long e = p * ld + k;
        const int a0 = min(max(4 * t0[e] - 2, 0), ow), a1 = min(max(4 * t1[e] + 2, 0), ow);
        const float c[2] = {(float)a0 / (float)ow * dims.x, (float)a1 / (float)ow * dims.x};
        s0[e] = c[0], s1[e] = c[1];
        int seg[2];
        spine_segments<2>(rows, nseg, c, seg);
        const float2 p00 = spine_point(rows, seg[0], c[0], -hh), p10 = spine_point(rows, seg[1], c[1], -hh);
        const float2 p11 = spine_point(rows, seg[1], c[1], hh), p01 = spine_point(rows, seg[0], c[0], hh);
        float4* q = reinterpret_cast<float4*>(cquads) + 2 * e;
        q[0] = make_float4(p00.x, p00.y, p10.x, p10.y);
        q[1] = make_float4(p11.x, p11.y, p01.x, p01.y);
    }
}

// One wave per line l (four lines per workgroup), one lane per word j of its chain.  The boundary behind the word at chain position q is
// b = start(word q + 1) - 0.5 len(gap q), two entries of the spine table; the boundaries do not decrease along a chain, so every word finds
// the two ends of its range by bisecting the characters' centres on its own: no scan across the lanes.
__global__ __launch_bounds__(256) void k_word_chars_chain(const float* __restrict__ spine, long wcap, const int* __restrict__ n_lines, long cap,
                                                          const int* __restrict__ line_offsets, const int* __restrict__ word_order, const int* __restrict__ plan,
                                                          long rows, int ld, const int* __restrict__ labels, const int* __restrict__ lens,
                                                          const float* __restrict__ s0, const float* __restrict__ s1, int space, int* __restrict__ word_chars) {
    const int lane = threadIdx.x & 63;
    const long l = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (l >= line_count(n_lines, cap)) return;
    const long p = plan[l * 8 + 6];
    if (p < 0 || p >= rows) return;
    int off, m;
    if (!line_range(line_offsets, l, wcap, off, m)) return;
    const int nch = min(max(lens[p], 0), ld);
    const int* lab = labels + p * ld;
    const float* c0 = s0 + p * ld;
    const float* c1 = s1 + p * ld;
    for (int j = lane; j < m; j += 64) {
        const long w = word_order[off + j];
        if (w < 0 || w >= wcap) continue;
        const float* row = spine + 16 * ((long)off + j);  // the word's row; +8 its gap, +16 the next word, -8 the gap before it
        const int first = j == 0 ? 0 : chars_below(c0, c1, nch, row[0] - 0.5f * row[-8 + 1]);
        const int end = j == m - 1 ? nch : chars_below(c0, c1, nch, row[16] - 0.5f * row[8 + 1]);
        store_word_range(lab, first, end, space, word_chars, w);
    }
}

}  // namespace

extern "C" {

int ocrs_line_spines(const float* words, long wcap, const int* n_lines, long cap, const int* line_offsets, const int* word_order, float* spine, float* line_dims,
                     hipStream_t st) {
    OCRS_CHECK_ARG(wcap >= 0 && cap >= 0 && cap <= wcap && cap < (1L << 29));
    if (cap == 0) return OCRS_OK;
    OCRS_CHECK_ARG(words && n_lines && line_offsets && word_order && spine && line_dims && aligned16(words) && aligned16(spine));
    OCRS_CHECK_ARG((reinterpret_cast<uintptr_t>(line_dims) & 7) == 0);
    hipLaunchKernelGGL(k_line_spines, dim3((unsigned)((cap + 3) / 4)), dim3(256), 0, st, words, wcap, n_lines, cap, line_offsets, word_order, spine, line_dims);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

int ocrs_rectify_chain(const unsigned char* page, int H, int W, const float* spine, const float* line_dims, const int* line_offsets, long wcap, const int* plan,
                       const long long* totals, long max_tiles, float* packed, long packed_floats, hipStream_t st) {
    OCRS_CHECK_ARG(H > 0 && W > 0 && wcap >= 0 && max_tiles >= 0 && max_tiles < (1L << 31) && packed_floats >= 0);
    if (max_tiles == 0) return OCRS_OK;
    OCRS_CHECK_ARG(page && spine && line_dims && line_offsets && plan && totals && packed && aligned16(spine) && aligned16(plan) && aligned16(packed));
    OCRS_CHECK_ARG((reinterpret_cast<uintptr_t>(line_dims) & 7) == 0);
    hipLaunchKernelGGL(k_rectify_chain, dim3((unsigned)max_tiles), dim3(256), 0, st, page, H, W, spine, line_dims, line_offsets, wcap, plan, totals, packed,
                       packed_floats);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

int ocrs_rectify_chain_pages(const unsigned char* pages, long pages_bytes, const long long* page_offs, const int* page_sizes, int B, const float* spine,
                             const float* line_dims, const int* line_offsets, long wcap, const int* page_of_line, const int* plan, const long long* totals,
                             long max_tiles, float* packed, long packed_floats, hipStream_t st) {
    OCRS_CHECK_ARG(B >= 0 && pages_bytes >= 0 && wcap >= 0 && max_tiles >= 0 && max_tiles < (1L << 31) && packed_floats >= 0);
    if (max_tiles == 0) return OCRS_OK;
    OCRS_CHECK_ARG(pages && page_offs && page_sizes && spine && line_dims && line_offsets && page_of_line && plan && totals && packed);
    OCRS_CHECK_ARG(aligned16(spine) && aligned16(plan) && aligned16(packed) && (reinterpret_cast<uintptr_t>(line_dims) & 7) == 0);
    hipLaunchKernelGGL(k_rectify_chain_pages, dim3((unsigned)max_tiles), dim3(256), 0, st, pages, pages_bytes, page_offs, page_sizes, B, spine, line_dims,
                       line_offsets, wcap, page_of_line, plan, totals, packed, packed_floats);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

int ocrs_char_boxes_chain(const float* spine, const float* line_dims, const int* line_offsets, long wcap, const int* plan, long cap, long rows, int ld,
                          const int* lens, const int* t0, const int* t1, float* s0, float* s1, float* char_quads, hipStream_t st) {
    OCRS_CHECK_ARG(wcap >= 0 && cap >= 0 && cap <= wcap && rows >= 0 && rows <= cap && rows < (1L << 31) && ld > 0);
    if (rows == 0) return OCRS_OK;
    OCRS_CHECK_ARG(spine && line_dims && line_offsets && plan && lens && t0 && t1 && s0 && s1 && char_quads && aligned16(spine) && aligned16(char_quads));
    OCRS_CHECK_ARG((reinterpret_cast<uintptr_t>(line_dims) & 7) == 0);
    hipLaunchKernelGGL(k_char_boxes_chain, dim3((unsigned)rows), dim3(64), 0, st, spine, line_dims, line_offsets, wcap, plan, cap, ld, lens, t0, t1, s0, s1,
                       char_quads);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

int ocrs_word_chars_chain(const float* spine, long wcap, const int* n_lines, long cap, const int* line_offsets, const int* word_order, const int* plan, long rows,
                          int ld, const int* labels, const int* lens, const float* s0, const float* s1, int space, int* word_chars, hipStream_t st) {
    OCRS_CHECK_ARG(wcap >= 0 && cap >= 0 && cap <= wcap && rows >= 0 && rows <= cap && cap < (1L << 31) && ld > 0);
    if (cap == 0 || rows == 0) return OCRS_OK;
    OCRS_CHECK_ARG(spine && n_lines && line_offsets && word_order && plan && labels && lens && s0 && s1 && word_chars);
    OCRS_CHECK_ARG(aligned16(spine) && (reinterpret_cast<uintptr_t>(word_chars) & 7) == 0);
    hipLaunchKernelGGL(k_word_chars_chain, dim3((unsigned)((cap + 3) / 4)), dim3(256), 0, st, spine, wcap, n_lines, cap, line_offsets, word_order, plan, rows, ld,
                       labels, lens, s0, s1, space, word_chars);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

}  // extern "C"
