// Page inference: the pixel work between the two models' eval forwards (ocrs_models/eval_detection.py:52-67 and the line-crop preparation
// of datasets/hiertext.py:271-294, here applied to detected word rectangles).
//
//   k_binarize_resize_nearest   binarize_mask + resize(.., NEAREST)   eval_detection.py:54-57   probabilities -> uint8 0/1 page mask
//   k_expand_quads              expand_quads(dist)                     postprocess.py:39-76       every rectangle edge moved outward
//   k_crop_plan                 (new) per-quad crop geometry, packed offsets, counting sort by output width; one workgroup
//   k_rectify_crops             (new) rotated rectangles cut out of the uint8 page, transform_image fused, bilinear
//   k_resize_aa_packed_{h,v}    resize(.., antialias=True) per crop    hiertext.py:288-294        + collate_samples' right padding
//
// Page batches: the same stages for B pages of different sizes at once.
//   k_binarize_resize_pages     k_binarize_resize_nearest per page into one zero-padded (B, Hmax, Wmax) canvas, padding included
//   k_gather_page_quads         (B, cap) quads with counts -> flat rows grouped by page, page_of_word, word_offs
//   k_rectify_crops_pages       k_rectify_crops with the page looked up per crop in a packed page store; both find the crop with
//                               crop_of_tile() and sample it with rectify_tile(), the one statement of the sampler
//
// All of them are small and byte-bound: no LDS tiles, no MFMA; coalesced 4..16-byte vector accesses; every count stays on the device.
#include "crop_frame.h"
#include "crop_sample.h"

namespace {

constexpr int kOwBins = 801;  // line_output_width() is clamped to [10, 800]

// ---- binarize + nearest resize -------------------------------------------------------------------------------------------------
// One lane = 16 consecutive output bytes of the flat (B, H, W) mask (the tensor base is 16-byte aligned, rows need not be): one b128 store.
// The source row pointer is recomputed only when the lane's run crosses into the next output row.
__global__ __launch_bounds__(256) void k_binarize_resize_nearest(const float* __restrict__ prob, uint8_t* __restrict__ out, int h, int w, int H, int W,
                                                                 long total, float threshold, float sy, float sx) {
    const long nchunks = (total + 15) / 16;
    for (long c = (long)blockIdx.x * 256 + threadIdx.x; c < nchunks; c += (long)gridDim.x * 256) {
        const long e = c * 16;
        long row = e / W;  // b * H + y
        int x = (int)(e - row * W);
        long b = row / H;
        int y = (int)(row - b * H);
        const float* src = prob + (b * h + min((int)floorf((float)y * sy), h - 1)) * (long)w;
        const int nv = (int)min(16L, total - e);
        unsigned wd[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if (k < nv) {
                const int xs = min((int)floorf((float)x * sx), w - 1);
                if (src[xs] > threshold) wd[k >> 2] |= 1u << (8 * (k & 3));
                if (++x == W) {
                    x = 0;
                    if (++y == H) y = 0, ++b;
                    src = prob + (b * h + min((int)floorf((float)y * sy), h - 1)) * (long)w;  // (past the last row: formed, never read)
                }
            }
        }
        if (nv == 16) {
            *reinterpret_cast<uint4*>(out + e) = make_uint4(wd[0], wd[1], wd[2], wd[3]);
        } else {
            for (int k = 0; k < nv; ++k) out[e + k] = (uint8_t)((wd[k >> 2] >> (8 * (k & 3))) & 0xff);
        }
    }
}

// The same per page into one canvas (B, Hmax, Wmax): inside (H_p, W_p) the byte k_binarize_resize_nearest writes for that page alone (the
// same float scales h / H_p and w / W_p, the same floorf and clamp), 0 outside.  One lane = 16 consecutive canvas bytes, padding included,
// taken one canvas row at a time: the page's size and scales are looked up per row piece, not per byte.
__global__ __launch_bounds__(256) void k_binarize_resize_pages(const float* __restrict__ prob, const int* __restrict__ page_sizes, uint8_t* __restrict__ out, int h,
                                                               int w, int Hmax, int Wmax, long total, float threshold) {
    const long nchunks = (total + 15) / 16;
    for (long c = (long)blockIdx.x * 256 + threadIdx.x; c < nchunks; c += (long)gridDim.x * 256) {
        const long e = c * 16;
        long row = e / Wmax;  // b * Hmax + y
        int x = (int)(e - row * Wmax);
        long b = row / Hmax;
        int y = (int)(row - b * Hmax);
        const int nv = (int)min(16L, total - e);
        unsigned long long lo = 0ULL, hi = 0ULL;  // bytes 0..7 and 8..15
        for (int k = 0; k < nv;) {
            const int run = min(nv - k, Wmax - x);  // the piece of row (b, y) from x on
            const int H = min(page_sizes[2 * b], Hmax), W = min(page_sizes[2 * b + 1], Wmax);
            if (y < H && x < W) {
                const float sy = (float)h / (float)H, sx = (float)w / (float)W;
                const float* src = prob + (b * h + min((int)floorf((float)y * sy), h - 1)) * (long)w;
                const int m = min(run, W - x);
                for (int q = 0; q < m; ++q) {
                    const int xs = min((int)floorf((float)(x + q) * sx), w - 1);
                    if (src[xs] > threshold) {
                        const int bit = 8 * (k + q);
                        if (bit < 64) lo |= 1ULL << bit; else hi |= 1ULL << (bit - 64);
                    }
                }
            }
            k += run, x += run;
            if (x == Wmax) {
                x = 0;
                if (++y == Hmax) y = 0, ++b;
            }
        }
        if (nv == 16) {
            *reinterpret_cast<uint4*>(out + e) = make_uint4((unsigned)lo, (unsigned)(lo >> 32), (unsigned)hi, (unsigned)(hi >> 32));
        } else {
            for (int k = 0; k < nv; ++k) out[e + k] = (uint8_t)(((k < 8 ? lo >> (8 * k) : hi >> (8 * (k - 8)))) & 0xff);
        }
    }
}

// ---- quad expansion --------------------------------------------------------------------------------------------------------------
// One lane = one quad (two 16-byte loads, two 16-byte stores).  fp64 inside, so the result is the correctly rounded fp32 of the rule.
__global__ __launch_bounds__(256) void k_expand_quads(const float* __restrict__ quads, float* __restrict__ out, const int* __restrict__ counts, long cap,
                                                      long total, float dist) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    if (counts) {
        const long b = i / cap;
        if (i - b * cap >= counts[b]) return;  // rows past the count are left untouched
    }
    const float4 a = reinterpret_cast<const float4*>(quads)[2 * i], c = reinterpret_cast<const float4*>(quads)[2 * i + 1];
    const double x0 = a.x, y0 = a.y, x1 = a.z, y1 = a.w, x2 = c.x, y2 = c.y, x3 = c.z, y3 = c.w;
    const double e1x = x1 - x0, e1y = y1 - y0, e2x = x2 - x1, e2y = y2 - y1;
    const double l1 = sqrt(e1x * e1x + e1y * e1y), l2 = sqrt(e2x * e2x + e2y * e2y);
    if (l1 == 0.0 && l2 == 0.0) {  // a point cannot be offset (postprocess.py:51-53)
        reinterpret_cast<float4*>(out)[2 * i] = a;
        reinterpret_cast<float4*>(out)[2 * i + 1] = c;
        return;
    }
    double ux = 0.0, uy = 0.0, vx = 0.0, vy = 0.0;
    if (l1 > 0.0) ux = e1x / l1, uy = e1y / l1;
    if (l2 > 0.0) vx = e2x / l2, vy = e2y / l2;
    if (l1 == 0.0) ux = vy, uy = -vx;  // zero-area ring: the missing axis is the normal of the other one
    if (l2 == 0.0) vx = -uy, vy = ux;
    const double cx = 0.25 * (x0 + x1 + x2 + x3), cy = 0.25 * (y0 + y1 + y2 + y3);
    const double ha = 0.5 * l1 + (double)dist, hb = 0.5 * l2 + (double)dist;
    const double ax = ha * ux, ay = ha * uy, bx = hb * vx, by = hb * vy;
    reinterpret_cast<float4*>(out)[2 * i] = make_float4((float)(cx - ax - bx), (float)(cy - ay - by), (float)(cx + ax - bx), (float)(cy + ay - by));
    reinterpret_cast<float4*>(out)[2 * i + 1] = make_float4((float)(cx + ax + bx), (float)(cy + ay + by), (float)(cx - ax + bx), (float)(cy - ay + by));
}

// ---- compaction of the per-page quads ---------------------------------------------------------------------------------------------
// grid (ceil(cap / 256), B): workgroup (c, b) copies rows c * 256 .. of page b to the flat rows that start at the sum of the earlier counts
// (B is small: every lane adds them up, one address per step).  Workgroup (0, 0) writes word_offs.  out == nullptr: word_offs only.
__device__ __forceinline__ long page_count(const int* __restrict__ counts, int b, long cap) { return min((long)max(counts[b], 0), cap); }
__global__ __launch_bounds__(256) void k_gather_page_quads(const float* __restrict__ quads, const int* __restrict__ counts, int B, long cap, float* __restrict__ out,
                                                           int* __restrict__ page_of_word, int* __restrict__ word_offs, long out_cap) {
    const int b = blockIdx.y;
    if (blockIdx.x == 0 && b == 0 && threadIdx.x == 0) {
        long run = 0;
        for (int q = 0; q < B; ++q) word_offs[q] = (int)run, run += page_count(counts, q, cap);
        word_offs[B] = (int)run;
    }
    if (!out) return;
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if ((long)blockIdx.x * 256 >= page_count(counts, b, cap)) return;  // (block-uniform, before the sum)
    long base = 0;
    for (int q = 0; q < b; ++q) base += page_count(counts, q, cap);
    if (r >= page_count(counts, b, cap) || base + r >= out_cap) return;
    const float4* src = reinterpret_cast<const float4*>(quads) + 2 * ((long)b * cap + r);
    float4* dst = reinterpret_cast<float4*>(out) + 2 * (base + r);
    dst[0] = src[0], dst[1] = src[1];
    page_of_word[base + r] = b;
}

// ---- crop frame: CropFrame / crop_frame(), the one statement of the geometry rule, live in crop_frame.h (char_spans.hip uses them too) ------

// hiertext.py:288-292 / input_pipeline.line_output_width, in the host's fp64 arithmetic
__device__ __forceinline__ int line_output_width(int h, int w, int OH) {
    const int ow = (int)((double)OH * ((double)w / (double)h));
    return min(kOwBins - 1, max(10, ow));
}

// Where crop i's (h, w) come from: the crop frame of a quad, or the (S, H) of a chain crop (line_chain.hip).
struct QuadSize {
    const float* __restrict__ quads;
    __device__ __forceinline__ int2 operator()(long i) const {
        const CropFrame f = crop_frame(quads + i * 8);
        return make_int2(f.h, f.w);
    }
};
struct DimsSize {
    const float* __restrict__ dims;  // [cap][2]: S, H
    __device__ __forceinline__ int2 operator()(long i) const {
        const float2 d = reinterpret_cast<const float2*>(dims)[i];
        return make_int2(crop_len(d.y), crop_len(d.x));
    }
};

// One workgroup walks the crops in index order, 256 at a time: geometry, three running prefix sums (packed elements, horizontal-pass
// elements, sampler tiles), a histogram of output widths; then a stable counting sort by output width (rank = bin start + earlier equals).
template <class Size>
__global__ __launch_bounds__(256) void k_crop_plan(const Size size, const int* __restrict__ count, long cap, int OH, int* __restrict__ plan,
                                                   long long* __restrict__ totals) {
    __shared__ int s_hist[kOwBins], s_cnt[kOwBins], s_ow[256];
    __shared__ long long s_scan[3][256];
    const int t = threadIdx.x;
    long n = cap;
    if (count) n = min((long)max(*count, 0), cap);
    for (int i = t; i < kOwBins; i += 256) s_hist[i] = 0, s_cnt[i] = 0;
    long long base[3] = {0, 0, 0};
    __syncthreads();
    for (long t0 = 0; t0 < n; t0 += 256) {
        const long i = t0 + t;
        long long v[3] = {0, 0, 0};
        int h = 0, w = 0, ow = 0;
        if (i < n) {
            const int2 hw2 = size(i);
            h = hw2.x, w = hw2.y;
            ow = line_output_width(h, w, OH);
            const long long hw = (long long)h * w;
            v[0] = (hw + 3) & ~3LL;  // every crop starts 16-byte aligned in the packed buffer
            v[1] = (long long)h * ow;
            v[2] = (hw + kTileElems - 1) / kTileElems;
            atomicAdd(&s_hist[ow], 1);
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) s_scan[q][t] = v[q];
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {  // inclusive scan
            long long add[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) add[q] = t >= o ? s_scan[q][t - o] : 0;
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 3; ++q) s_scan[q][t] += add[q];
            __syncthreads();
        }
        if (i < n) {
            *reinterpret_cast<int4*>(plan + i * 8) = make_int4(h, w, ow, (int)(base[0] + s_scan[0][t] - v[0]));
            *reinterpret_cast<int2*>(plan + i * 8 + 4) = make_int2((int)(base[1] + s_scan[1][t] - v[1]), (int)(base[2] + s_scan[2][t] - v[2]));
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) base[q] += s_scan[q][255];
        __syncthreads();
    }
    for (int i = t; i < kOwBins; i += 256) totals[4 + i] = s_hist[i];
    if (t == 0) {
        totals[0] = n, totals[1] = base[0], totals[2] = base[1], totals[3] = base[2];
    }
    __syncthreads();
    if (t == 0) {  // bin starts
        int run = 0;
        for (int i = 0; i < kOwBins; ++i) {
            const int c = s_hist[i];
            s_hist[i] = run;
            run += c;
        }
    }
    __syncthreads();
    for (long t0 = 0; t0 < n; t0 += 256) {
        const long i = t0 + t;
        const int ow = i < n ? plan[i * 8 + 2] : -1;  // written by this same lane above
        s_ow[t] = ow;
        __syncthreads();
        if (i < n) {
            int k = 0;
            for (int j = 0; j < t; ++j) k += s_ow[j] == ow;
            const int r = s_hist[ow] + s_cnt[ow] + k;
            plan[i * 8 + 6] = r;         // position of quad i in output-width order
            plan[(long)r * 8 + 7] = (int)i;  // and the quad at position r
        }
        __syncthreads();
        if (i < n) atomicAdd(&s_cnt[ow], 1);
        __syncthreads();
    }
}

// ---- rectification -----------------------------------------------------------------------------------------------------------------
// One workgroup = one tile of kTileElems consecutive elements of one crop; the crop is found by bisecting the plan's tile prefix and its
// frame is computed once (wave-uniform: scalar registers).  One lane = 4 consecutive samples -> one 16-byte store; the taps are byte loads
// of the page, which stays in L2 (a page is a few MB).

// (kTileElems, crop_of_tile() and the tap sample_u8() are crop_sample.h's: the chain sampler of line_chain.hip uses them too)
// The sampler: this lane's 4 samples of tile `tile` of crop `crop`, taken from the (H, W) page.
__device__ __forceinline__ void rectify_tile(const uint8_t* __restrict__ page, int H, int W, const float* __restrict__ quads, const int* __restrict__ plan, long crop,
                                             long long tile, float* __restrict__ packed, long packed_floats) {
    const CropFrame f = crop_frame(quads + crop * 8);
    const int4 pl = *reinterpret_cast<const int4*>(plan + crop * 8);  // h, w, ow, packed offset
    const int h = pl.x, w = pl.y;
    const long hw = (long)h * w;
    const long e0 = (long)(tile - plan[crop * 8 + 5]) * kTileElems + threadIdx.x * 4;
    if (e0 >= hw || (long)pl.w + e0 + 4 > packed_floats) return;
    const float vx = -f.uy, vy = f.ux;
    float out[4];
    int y = (int)(e0 / w), x = (int)(e0 - (long)y * w);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float val = 0.0f;
        if (e0 + k < hw) {
            const float su = ((float)x + 0.5f) / (float)w * f.lng, sv = ((float)y + 0.5f) / (float)h * f.sht;
            val = sample_u8(page, H, W, f.ox + su * f.ux + sv * vx, f.oy + su * f.uy + sv * vy);
            if (++x == w) x = 0, ++y;
        }
        out[k] = val;
    }
    *reinterpret_cast<float4*>(packed + pl.w + e0) = make_float4(out[0], out[1], out[2], out[3]);
}

__global__ __launch_bounds__(256) void k_rectify_crops(const uint8_t* __restrict__ page, int H, int W, const float* __restrict__ quads,
                                                       const int* __restrict__ plan, const long long* __restrict__ totals, float* __restrict__ packed,
                                                       long packed_floats) {
    const long long tile = blockIdx.x;
    const long n = (long)totals[0];
    if (n <= 0 || tile >= totals[3]) return;
    rectify_tile(page, H, W, quads, plan, crop_of_tile(plan, n, tile), tile, packed, packed_floats);
}

// The same from a store of pages: the crop comes from page page_of_quad[crop], whose pointer and size are looked up once per workgroup
// (wave-uniform, like the frame), so a crop's bytes are those it gets from ocrs_rectify_crops on its own page.
__global__ __launch_bounds__(256) void k_rectify_crops_pages(const uint8_t* __restrict__ pages, long pages_bytes, const long long* __restrict__ page_offs,
                                                             const int* __restrict__ page_sizes, int B, const float* __restrict__ quads,
                                                             const int* __restrict__ page_of_quad, const int* __restrict__ plan,
                                                             const long long* __restrict__ totals, float* __restrict__ packed, long packed_floats) {
    const long long tile = blockIdx.x;
    const long n = (long)totals[0];
    if (n <= 0 || tile >= totals[3]) return;
    const long crop = crop_of_tile(plan, n, tile);
    const int pg = page_of_quad[crop];
    if ((unsigned)pg >= (unsigned)B) return;
    const int H = page_sizes[2 * pg], W = page_sizes[2 * pg + 1];
    const long long poff = page_offs[pg];
    if (H <= 0 || W <= 0 || poff < 0 || poff + (long long)H * W > pages_bytes) return;  // a page that is not inside the store is not read
    rectify_tile(pages + poff, H, W, quads, plan, crop, tile, packed, packed_floats);
}

// ---- antialiased resize of the packed crops into padded batches ------------------------------------------------------------------
// Same two passes in the same order as ocrs_resize_aa (horizontal, then vertical), through the same aa_span / aa_dot: same bits.
// crop i: packed (h, w) -> ws (h, ow).  grid (cap, ceil(800 / 256)); one lane = one output column, its span computed once for all rows.
__global__ __launch_bounds__(256) void k_resize_aa_packed_h(const float* __restrict__ packed, const int* __restrict__ plan, const int* __restrict__ count,
                                                            float* __restrict__ ws, long ws_floats) {
    const long i = blockIdx.x;
    if (count && i >= *count) return;
    const int4 pl = *reinterpret_cast<const int4*>(plan + i * 8);
    const int h = pl.x, w = pl.y, ow = pl.z;
    const long hoff = plan[i * 8 + 4];
    const int ox = blockIdx.y * 256 + threadIdx.x;
    if (ox >= ow || hoff + (long)h * ow > ws_floats) return;
    const AaSpan s = aa_span(ox, w, (float)w / (float)ow);
    const float* src = packed + pl.w + s.lo;
    float* dst = ws + hoff + ox;
    for (int y = 0; y < h; ++y) dst[(size_t)y * ow] = aa_dot(s, src + (size_t)y * w, 1);
}
// crop i: ws (h, ow) -> row `slot` of its chunk's (n, 1, OH, Wpad) batch, pad columns included.  grid (cap, OH); the span is block-uniform.
__global__ __launch_bounds__(256) void k_resize_aa_packed_v(const float* __restrict__ ws, const int* __restrict__ plan, const int* __restrict__ count,
                                                            const long long* __restrict__ chunks, int nchunks, int max_batch, float* __restrict__ out,
                                                            long out_floats, int OH) {
    const long i = blockIdx.x;
    if (count && i >= *count) return;
    const int h = plan[i * 8], ow = plan[i * 8 + 2], r = plan[i * 8 + 6];
    const long hoff = plan[i * 8 + 4];
    const int c = r / max_batch, slot = r - c * max_batch, oy = blockIdx.y;
    if (c >= nchunks) return;
    const long long Wpad = chunks[2 * c + 1];
    const long long row = chunks[2 * c] + ((long long)slot * OH + oy) * Wpad;
    if (row < 0 || row + Wpad > out_floats) return;
    const AaSpan s = aa_span(oy, h, (float)h / (float)OH);
    const float* src = ws + hoff + (size_t)s.lo * ow;
    for (int x = threadIdx.x; x < Wpad; x += 256) out[row + x] = x < ow ? aa_dot(s, src + x, ow) : 0.0f;  // pad value 0.0 (train_rec.py:295)
}

}  // namespace

extern "C" {

int ocrs_binarize_resize_nearest(const float* prob, unsigned char* out, int B, int h, int w, int H, int W, float threshold, hipStream_t st) {
    OCRS_CHECK_ARG(B >= 0 && h > 0 && w > 0 && H > 0 && W > 0);
    const long total = (long)B * H * W;
    if (total == 0) return OCRS_OK;
    OCRS_CHECK_ARG(prob && out && aligned16(out));
    long g = ((total + 15) / 16 + 255) / 256;
    g = g > kNumCU * 8 ? kNumCU * 8 : g;
    hipLaunchKernelGGL(k_binarize_resize_nearest, dim3((unsigned)g), dim3(256), 0, st, prob, out, h, w, H, W, total, threshold, (float)h / (float)H,
                       (float)w / (float)W);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

int ocrs_expand_quads(const float* quads, float* out, const int* counts, int B, long cap, float dist, hipStream_t st) {
    OCRS_CHECK_ARG(B >= 0 && cap >= 0);
    const long total = (long)B * cap;
    if (total == 0) return OCRS_OK;
    OCRS_CHECK_ARG(quads && out && aligned16(quads) && aligned16(out) && total < (1L << 31));
    hipLaunchKernelGGL(k_expand_quads, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, quads, out, counts, cap, total, dist);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

int ocrs_crop_plan(const float* quads, const int* count, long cap, int output_height, int* plan, long long* totals, hipStream_t st) {
    OCRS_CHECK_ARG(cap >= 0 && cap <= (1L << 24) && output_height > 0 && output_height <= 4096 && totals && aligned16(totals));
    OCRS_CHECK_ARG(cap == 0 || (quads && plan && aligned16(quads) && aligned16(plan)));
    hipLaunchKernelGGL(k_crop_plan<QuadSize>, dim3(1), dim3(256), 0, st, QuadSize{quads}, count, cap, output_height, plan, totals);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

// section "chain crops": the same plan from the (S, H) of ocrs_line_spines
int ocrs_crop_plan_dims(const float* line_dims, const int* count, long cap, int output_height, int* plan, long long* totals, hipStream_t st) {
    OCRS_CHECK_ARG(cap >= 0 && cap <= (1L << 24) && output_height > 0 && output_height <= 4096 && totals && aligned16(totals));
    OCRS_CHECK_ARG(cap == 0 || (line_dims && plan && aligned16(line_dims) && aligned16(plan)));
    hipLaunchKernelGGL(k_crop_plan<DimsSize>, dim3(1), dim3(256), 0, st, DimsSize{line_dims}, count, cap, output_height, plan, totals);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

int ocrs_rectify_crops(const unsigned char* page, int H, int W, const float* quads, const int* plan, const long long* totals, long max_tiles, float* packed,
                       long packed_floats, hipStream_t st) {
    OCRS_CHECK_ARG(H > 0 && W > 0 && max_tiles >= 0 && max_tiles < (1L << 31) && packed_floats >= 0);
    if (max_tiles == 0) return OCRS_OK;
    OCRS_CHECK_ARG(page && quads && plan && totals && packed && aligned16(quads) && aligned16(plan) && aligned16(packed));
    hipLaunchKernelGGL(k_rectify_crops, dim3((unsigned)max_tiles), dim3(256), 0, st, page, H, W, quads, plan, totals, packed, packed_floats);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

// ---- page batches ------------------------------------------------------------------------------------------------------------------
int ocrs_binarize_resize_pages(const float* prob, const int* page_sizes, unsigned char* out, int B, int h, int w, int Hmax, int Wmax, float threshold,
                               hipStream_t st) {
    OCRS_CHECK_ARG(B >= 0 && h > 0 && w > 0 && Hmax > 0 && Wmax > 0);
    const long total = (long)B * Hmax * Wmax;
    if (total == 0) return OCRS_OK;
    OCRS_CHECK_ARG(prob && page_sizes && out && aligned16(out));
    long g = ((total + 15) / 16 + 255) / 256;
    g = g > kNumCU * 8 ? kNumCU * 8 : g;
    hipLaunchKernelGGL(k_binarize_resize_pages, dim3((unsigned)g), dim3(256), 0, st, prob, page_sizes, out, h, w, Hmax, Wmax, total, threshold);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

int ocrs_gather_page_quads(const float* quads, const int* counts, int B, long cap, float* out, int* page_of_word, int* word_offs, long out_cap, hipStream_t st) {
    OCRS_CHECK_ARG(B >= 0 && B <= 65535 && cap >= 0 && out_cap >= 0 && (long)B * cap < (1L << 31) && word_offs);
    OCRS_CHECK_ARG(B == 0 || counts);
    OCRS_CHECK_ARG(!out || out_cap == 0 || (quads && page_of_word && aligned16(quads) && aligned16(out)));
    const bool rows = out && out_cap > 0 && cap > 0 && B > 0;
    const long gx = rows ? (cap + 255) / 256 : 1;
    hipLaunchKernelGGL(k_gather_page_quads, dim3((unsigned)gx, (unsigned)(B > 0 ? B : 1)), dim3(256), 0, st, quads, counts, B, cap, rows ? out : nullptr, page_of_word,
                       word_offs, out_cap);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

int ocrs_rectify_crops_pages(const unsigned char* pages, long pages_bytes, const long long* page_offs, const int* page_sizes, int B, const float* quads,
                             const int* page_of_quad, const int* plan, const long long* totals, long max_tiles, float* packed, long packed_floats,
                             hipStream_t st) {
    OCRS_CHECK_ARG(B >= 0 && pages_bytes >= 0 && max_tiles >= 0 && max_tiles < (1L << 31) && packed_floats >= 0);
    if (max_tiles == 0) return OCRS_OK;
    OCRS_CHECK_ARG(pages && page_offs && page_sizes && quads && page_of_quad && plan && totals && packed && aligned16(quads) && aligned16(plan) && aligned16(packed));
    hipLaunchKernelGGL(k_rectify_crops_pages, dim3((unsigned)max_tiles), dim3(256), 0, st, pages, pages_bytes, page_offs, page_sizes, B, quads, page_of_quad, plan,
                       totals, packed, packed_floats);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

long ocrs_resize_aa_packed_ws_floats(long hpass_floats) { return hpass_floats > 0 ? (hpass_floats + 3) & ~3L : 0; }

int ocrs_resize_aa_packed(const float* packed, const int* plan, const int* count, long cap, const long long* chunks, int nchunks, int max_batch, float* ws,
                          long ws_floats, float* out, long out_floats, int output_height, hipStream_t st) {
    OCRS_CHECK_ARG(cap >= 0 && cap < (1L << 31) && nchunks >= 0 && max_batch > 0 && ws_floats >= 0 && out_floats >= 0);
    OCRS_CHECK_ARG(output_height > 0 && output_height <= 65535);
    if (cap == 0 || nchunks == 0) return OCRS_OK;
    OCRS_CHECK_ARG(packed && plan && chunks && ws && out && aligned16(plan));
    hipLaunchKernelGGL(k_resize_aa_packed_h, dim3((unsigned)cap, (kOwBins + 254) / 256), dim3(256), 0, st, packed, plan, count, ws, ws_floats);
    hipLaunchKernelGGL(k_resize_aa_packed_v, dim3((unsigned)cap, output_height), dim3(256), 0, st, (const float*)ws, plan, count, chunks, nchunks, max_batch, out,
                       out_floats, output_height);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

}  // extern "C"
