// Detection training data (ocrs_models/datasets/hiertext.py:22-130, ddi100.py:34-107, datasets/util.py:54-110): the pages of the dataset
// live in HBM as one packed uint8 buffer with their word polygons (Python: ocrs_models_amd/datasets.py); a batch is gathered from it and
// every page's text mask is rasterised next to it.
//   k_shrink       shrink_polygon(poly, dist) once per store, one thread per polygon, fp64, by the project's own rule (the host
//                  restatement is tests/detdata_ref.py, whose operation order this mirrors), truncated as PIL takes float coordinates
//   k_page_batch   generate_mask(width, height, polys) = the union of PIL's polygon fill over the page's shrunk polygons (csrc/poly_fill.h),
//                  plus the byte copy of the page, for B store indices, in the packed layout ocrs_augment_det reads
// k_page_batch: one 64-lane workgroup per (page, row).  The page's polygons are sorted by y_min at store construction and a table per band
// of 16 rows gives the slice of them that can touch the band, so a row looks at its neighbours only.  Each lane takes ONE polygon of the
// slice (PIL's scanline is sequential per polygon, but the polygons of a row are independent: 64 of them run side by side) and ORs its
// spans into a bitmap of the row in LDS; polygons of more than kSmallVerts vertices go one at a time through the large scratch.  The row's
// bytes are then written once from the bitmap.  No atomics on global memory, no allocation, no host synchronisation.
#include "poly_fill.h"

// k_shrink must round as the host rule does (one rounding per operation, no fused multiply-add), and the fill needs the same for PIL's
// edge arithmetic: said here as well, so that neither depends on what an included file leaves in force
#pragma clang fp contract(off)

namespace {

constexpr int kSmallVerts = 8;   // a shrunk word quad has 4 vertices, 8 if every corner is bevelled
constexpr int kBandRows = 16;    // rows per entry of the band table (ocrs_models_amd/datasets.py builds it)
constexpr double kMaxOffsetCoord = 1048576.0;  // a shrunk ring that leaves +-2^20 is skipped (its integer truncation must be defined)

// ---- shrink ----------------------------------------------------------------------------------------------------------------------
// Edge i of the ring w (m vertices, {x, y, _} triples): its integer direction and the unit normal that points into the polygon,
// s * (-dy, dx) / len.  An axis-aligned edge has the components 0 and +-1 exactly.
__device__ void edge_normal(const int* w, int m, int s, int i, int& dx, int& dy, double& nx, double& ny) {
    const int j = i + 1 == m ? 0 : i + 1;
    dx = w[3 * j] - w[3 * i];
    dy = w[3 * j + 1] - w[3 * i + 1];
    if (dx == 0) {
        nx = dy > 0 ? (double)-s : (double)s;
        ny = 0.0;
    } else if (dy == 0) {
        nx = 0.0;
        ny = dx > 0 ? (double)s : (double)-s;
    } else {
        const double len = __dsqrt_rn((double)((long long)dx * dx + (long long)dy * dy));
        nx = (double)(-s * dy) / len;
        ny = (double)(s * dx) / len;
    }
}

// Output of vertex i: 0 = the ring is skipped (anti-parallel edges), 1 = the mitre point a, 2 = the bevel points a, b.
__device__ int corner(const int* w, int m, int s, double dist, int i, double2& a, double2& b) {
    int dx0, dy0, dx1, dy1;
    double n0x, n0y, n1x, n1y;
    edge_normal(w, m, s, i == 0 ? m - 1 : i - 1, dx0, dy0, n0x, n0y);
    edge_normal(w, m, s, i, dx1, dy1, n1x, n1y);
    const double vx = (double)w[3 * i], vy = (double)w[3 * i + 1];
    const long long cr = (long long)dx0 * dy1 - (long long)dy0 * dx1;
    if (cr == 0) {
        if ((long long)dx0 * dx1 + (long long)dy0 * dy1 <= 0) return 0;
        a = make_double2(vx + dist * n1x, vy + dist * n1y);
        return 1;
    }
    const double c = n0x * n1x + n0y * n1y;
    const double den = 1.0 + c;
    if ((long long)s * cr < 0 && den * 25.0 < 2.0) {  // reflex, and the mitre would be longer than 5 dist
        a = make_double2(vx + dist * n0x, vy + dist * n0y);
        b = make_double2(vx + dist * n1x, vy + dist * n1y);
        return 2;
    }
    if (dx0 == 0 || dx1 == 0) {  // a vertical edge fixes x exactly; the other edge's line gives y
        const double ax = dx0 == 0 ? n0x : n1x, ox = dx0 == 0 ? n1x : n0x, oy = dx0 == 0 ? n1y : n0y;
        const double tx = dist * ax;
        a = make_double2(vx + tx, vy + (dist - ox * tx) / oy);
        return 1;
    }
    if (dy0 == 0 || dy1 == 0) {  // a horizontal edge fixes y exactly
        const double ay = dy0 == 0 ? n0y : n1y, ox = dy0 == 0 ? n1x : n0x, oy = dy0 == 0 ? n1y : n0y;
        const double ty = dist * ay;
        a = make_double2(vx + (dist - oy * ty) / ox, vy + ty);
        return 1;
    }
    const double mm = dist / den;
    a = make_double2(vx + mm * (n0x + n1x), vy + mm * (n0y + n1y));
    return 1;
}

__global__ __launch_bounds__(64) void k_shrink(const int* __restrict__ verts, const long long* __restrict__ vert_offs,
                                               const int* __restrict__ vert_counts, int n_polys, double dist, int* __restrict__ ws,
                                               double* __restrict__ out_xy, int* __restrict__ out_verts, int* __restrict__ out_counts,
                                               int* __restrict__ out_rows) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= n_polys) return;
    const long long off = vert_offs[p];
    int n = vert_counts[p];
    n = n < 0 ? 0 : (n > kMaxVerts ? kMaxVerts : n);
    const int* v = verts + 2 * off;
    int* w = ws + 3 * off;
    double* oxy = out_xy + 4 * off;  // room for 2 n points
    int* ov = out_verts + 4 * off;
    int cnt = 0;
    if (dist == 0.0) {  // generate_mask's bypass: the vertices as they are
        for (int i = 0; i < n; ++i) {
            oxy[2 * i] = (double)v[2 * i];
            oxy[2 * i + 1] = (double)v[2 * i + 1];
        }
        cnt = n;
    } else {
        int m = 0;
        for (int i = 0; i < n; ++i) {  // consecutive duplicates
            const int x = v[2 * i], y = v[2 * i + 1];
            if (m && w[3 * (m - 1)] == x && w[3 * (m - 1) + 1] == y) continue;
            w[3 * m] = x;
            w[3 * m + 1] = y;
            ++m;
        }
        while (m > 1 && w[3 * (m - 1)] == w[0] && w[3 * (m - 1) + 1] == w[1]) --m;  // a closing vertex
        long long area2 = 0;
        for (int i = 0; i < m; ++i) {
            const int j = i + 1 == m ? 0 : i + 1;
            area2 += (long long)w[3 * i] * w[3 * j + 1] - (long long)w[3 * j] * w[3 * i + 1];
        }
        bool ok = m >= 3 && area2 != 0;
        const int s = area2 > 0 ? 1 : -1;
        for (int i = 0; ok && i < m; ++i) {
            double2 a, b;
            const int k = corner(w, m, s, dist, i, a, b);
            if (k == 0) {
                ok = false;
                break;
            }
            w[3 * i + 2] = cnt;
            oxy[2 * cnt] = a.x;
            oxy[2 * cnt + 1] = a.y;
            ++cnt;
            if (k == 2) {
                oxy[2 * cnt] = b.x;
                oxy[2 * cnt + 1] = b.y;
                ++cnt;
            }
        }
        for (int i = 0; ok && i < m; ++i) {  // an output edge that points against its input edge: the edge has collapsed
            const int j = i + 1 == m ? 0 : i + 1;
            const int ia = (j == 0 ? cnt : w[3 * j + 2]) - 1, ib = w[3 * j + 2];
            const double ex = oxy[2 * ib] - oxy[2 * ia], ey = oxy[2 * ib + 1] - oxy[2 * ia + 1];
            const double dot = ex * (double)(w[3 * j] - w[3 * i]) + ey * (double)(w[3 * j + 1] - w[3 * i + 1]);
            if (!(dot > 0.0)) ok = false;
        }
        if (ok) {  // the ring has flipped, or left the range
            double acc = 0.0;
            for (int k = 0; k < cnt; ++k) {
                const int j = k + 1 == cnt ? 0 : k + 1;
                acc += oxy[2 * k] * oxy[2 * j + 1] - oxy[2 * j] * oxy[2 * k + 1];
                if (!(fabs(oxy[2 * k]) <= kMaxOffsetCoord) || !(fabs(oxy[2 * k + 1]) <= kMaxOffsetCoord)) ok = false;
            }
            if (!(acc * (double)s > 0.0)) ok = false;
        }
        if (!ok) cnt = 0;
    }
    int ymin = 0, ymax = -1;
    for (int k = 0; k < cnt; ++k) {  // (int): PIL's conversion of a float coordinate
        const int x = (int)oxy[2 * k], y = (int)oxy[2 * k + 1];
        ov[2 * k] = x;
        ov[2 * k + 1] = y;
        ymin = k ? min(ymin, y) : y;
        ymax = k ? max(ymax, y) : y;
    }
    out_counts[p] = cnt > kMaxVerts ? -1 : cnt;  // (-1: the host refuses the store)
    out_rows[2 * p] = ymin;
    out_rows[2 * p + 1] = ymax;
}

// ---- page batch ------------------------------------------------------------------------------------------------------------------
struct PageScratch {
    union {
        PolyScratch<kSmallVerts> small[64];
        RowScratch large;
    };
};

// ORs the span [lo, hi] (already clipped to the row) into the row's bitmap; one lane.
__device__ __forceinline__ void or_span(unsigned* bits, int lo, int hi) {
    const int w0 = lo >> 5, w1 = hi >> 5;
    const unsigned m0 = 0xffffffffu << (lo & 31), m1 = 0xffffffffu >> (31 - (hi & 31));
    if (w0 == w1) {
        atomicOr(&bits[w0], m0 & m1);  // (LDS)
        return;
    }
    atomicOr(&bits[w0], m0);
    for (int w = w0 + 1; w < w1; ++w) atomicOr(&bits[w], 0xffffffffu);
    atomicOr(&bits[w1], m1);
}

__device__ __forceinline__ unsigned spread4(unsigned nib) {  // bits 0..3 -> bytes 0..3
    return (nib & 1u) | ((nib & 2u) << 7) | ((nib & 4u) << 14) | ((nib & 8u) << 21);
}

// polys [n_polys][4] = {first vertex, vertex count, y_min, y_max}, each page's sorted by y_min; bands [..][2] = the slice [lo, hi) of polys
// that can touch a band of kBandRows rows, page l's bands from band_offs[l]
__global__ __launch_bounds__(64) void k_page_batch(const uint8_t* __restrict__ pixels, const long long* __restrict__ px_offs,
                                                   const int* __restrict__ sizes, const int* __restrict__ verts, long long n_verts,
                                                   const int* __restrict__ polys, int n_polys, const long long* __restrict__ band_offs,
                                                   const int* __restrict__ bands, int N, const int* __restrict__ indices,
                                                   const long long* __restrict__ batch_offs, uint8_t* __restrict__ pages,
                                                   uint8_t* __restrict__ masks) {
    __shared__ PageScratch s;
    extern __shared__ unsigned bits[];  // (W + 31) / 32 + 1 words
    const int b = blockIdx.y, y = blockIdx.x, t = threadIdx.x;
    int l = indices[b];
    l = l < 0 ? 0 : (l >= N ? N - 1 : l);  // (indices are checked on the host; never read outside the store)
    const int H = sizes[2 * l], W = sizes[2 * l + 1];
    if (y >= H) return;
    const long long at = batch_offs[b] + (long long)y * W;
    const uint8_t* src = pixels + px_offs[l] + (long long)y * W;
    uint8_t* dst = pages + at;
    uint8_t* mdst = masks + at;
    // the part of the row that both sides can move 16 bytes at a time (page and batch offsets are multiples of 16, so the two agree)
    const int head = min(W, (int)((16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15));
    const int nv = (W - head) >> 4;
    const bool vec = ((reinterpret_cast<uintptr_t>(src) ^ reinterpret_cast<uintptr_t>(dst)) & 15) == 0 &&
                     ((reinterpret_cast<uintptr_t>(mdst) ^ reinterpret_cast<uintptr_t>(dst)) & 15) == 0;
    if (vec) {
        for (int x = t; x < head; x += 64) dst[x] = src[x];
        for (int i = t; i < nv; i += 64) reinterpret_cast<uint4*>(dst + head)[i] = reinterpret_cast<const uint4*>(src + head)[i];
        for (int x = head + (nv << 4) + t; x < W; x += 64) dst[x] = src[x];
    } else {
        for (int x = t; x < W; x += 64) dst[x] = src[x];
    }

    const int words = ((W + 31) >> 5) + 1;
    for (int i = t; i < words; i += 64) bits[i] = 0;
    __syncthreads();
    const long long band = band_offs[l] + y / kBandRows;
    const int p0 = max(bands[2 * band], 0), p1 = min(bands[2 * band + 1], n_polys);
    for (int base = p0; base < p1; base += 64) {
        const int p = base + t;
        int cnt = 0;
        long long first = 0;
        if (p < p1) {
            const int4 rec = reinterpret_cast<const int4*>(polys)[p];
            if (rec.z <= y && y <= rec.w && rec.y > 0 && rec.y <= kMaxVerts && rec.x >= 0 && (long long)rec.x + rec.y <= n_verts) {
                cnt = rec.y;
                first = rec.x;
            }
        }
        if (cnt > 0 && cnt <= kSmallVerts) {
            PolyScratch<kSmallVerts>& mine = s.small[t];
            for (int i = 0; i < cnt; ++i) mine.v[i] = make_int2(verts[2 * (first + i)], verts[2 * (first + i) + 1]);
            row_spans(mine, cnt, H, y);
            for (int k = 0; k < mine.ns; ++k) {
                const int lo = max(mine.span[k].x, 0), hi = min(mine.span[k].y, W - 1);
                if (lo <= hi) or_span(bits, lo, hi);
            }
        }
        unsigned long long big = __ballot(cnt > kSmallVerts);
        while (big) {  // (uniform: every lane sees the same ballot)
            const int lane = __ffsll((long long)big) - 1;
            big &= big - 1;
            const int bn = __shfl(cnt, lane);
            const long long bf = __shfl(first, lane);
            __syncthreads();  // the small scratches share the large one's LDS
            for (int i = t; i < bn; i += 64) s.large.v[i] = make_int2(verts[2 * (bf + i)], verts[2 * (bf + i) + 1]);
            __syncthreads();
            if (t == 0) row_spans(s.large, bn, H, y);
            __syncthreads();
            for (int k = t; k < s.large.ns; k += 64) {
                const int lo = max(s.large.span[k].x, 0), hi = min(s.large.span[k].y, W - 1);
                if (lo <= hi) or_span(bits, lo, hi);
            }
        }
        __syncthreads();
    }
    __syncthreads();
    if (vec) {
        for (int x = t; x < head; x += 64) mdst[x] = (bits[x >> 5] >> (x & 31)) & 1u;
        for (int i = t; i < nv; i += 64) {
            const int x = head + (i << 4);
            const unsigned long long two = (unsigned long long)bits[x >> 5] | ((unsigned long long)bits[(x >> 5) + 1] << 32);
            const unsigned m = (unsigned)(two >> (x & 31)) & 0xffffu;
            reinterpret_cast<uint4*>(mdst + head)[i] = make_uint4(spread4(m & 15u), spread4((m >> 4) & 15u), spread4((m >> 8) & 15u), spread4(m >> 12));
        }
        for (int x = head + (nv << 4) + t; x < W; x += 64) mdst[x] = (bits[x >> 5] >> (x & 31)) & 1u;
    } else {
        for (int x = t; x < W; x += 64) mdst[x] = (bits[x >> 5] >> (x & 31)) & 1u;
    }
}

}  // namespace

extern "C" {

int ocrs_shrink_polygons(const int* vertices, const long long* vertex_offs, const int* vertex_counts, int n, double dist, int* ws, double* out_xy,
                         int* out_vertices, int* out_counts, int* out_rows, hipStream_t st) {
    OCRS_CHECK_ARG(n >= 0 && dist >= 0.0);
    if (n == 0) return OCRS_OK;
    OCRS_CHECK_ARG(vertices && vertex_offs && vertex_counts && ws && out_xy && out_vertices && out_counts && out_rows);
    hipLaunchKernelGGL(k_shrink, dim3((n + 63) / 64), dim3(64), 0, st, vertices, vertex_offs, vertex_counts, n, dist, ws, out_xy, out_vertices,
                       out_counts, out_rows);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

int ocrs_page_batch(const void* pixels_u8, const long long* pixel_offs, const int* sizes, const int* vertices, long n_vertices, const int* polys,
                    int n_polys, const long long* band_offs, const int* bands, int N, const int* indices, int B, int max_h, int max_w,
                    const long long* batch_offs, void* out_pages_u8, void* out_masks_u8, hipStream_t st) {
    OCRS_CHECK_ARG(B >= 0 && B <= 65535 && N >= 1 && n_polys >= 0 && n_vertices >= 0);
    if (B == 0) return OCRS_OK;
    OCRS_CHECK_ARG(pixels_u8 && pixel_offs && sizes && band_offs && bands && indices && batch_offs && out_pages_u8 && out_masks_u8 &&
                   max_h >= 1 && max_h <= 65535 && max_w >= 1 && max_w <= 65535);
    OCRS_CHECK_ARG(n_polys == 0 || (vertices && polys));
    const size_t lds = (size_t)(((max_w + 31) >> 5) + 1) * sizeof(unsigned);
    hipLaunchKernelGGL(k_page_batch, dim3(max_h, B), dim3(64), lds, st, static_cast<const uint8_t*>(pixels_u8), pixel_offs, sizes, vertices,
                       (long long)n_vertices, polys, n_polys, band_offs, bands, N, indices, batch_offs, static_cast<uint8_t*>(out_pages_u8),
                       static_cast<uint8_t*>(out_masks_u8));
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

}  // extern "C"
