// Recognition training data (ocrs_models/datasets/hiertext.py:238-274): the line crops of the dataset live in HBM as one packed uint8
// buffer (Python: ocrs_models_amd/datasets.py); a batch is gathered from it and every crop's polygon mask is rasterised next to it.
//   k_line_mask    generate_mask(w, h, [poly], shrink_dist=0.0) = PIL's ImageDraw.polygon(poly, fill="white", outline=None) on a mode "1"
//                  image, restated operation by operation (tests/hiertext_ref.py is the host restatement this was ported from)
//   k_line_batch   the same plus the coalesced byte copy of the crop, for B store indices, in the packed layout ocrs_augment_lines reads
// One 64-lane workgroup per (sample, row).  PIL's fill is a sequential scanline algorithm whose result depends on the edge order, so lane 0
// builds and sorts the row's crossings in LDS exactly in that order; then all lanes write the row's bytes.  No atomics, no allocation.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxVerts = 512;  // per polygon; the host refuses a longer one (ocrs_models_amd/datasets.py)

struct RowScratch {
    int2 v[kMaxVerts];
    float xx[2 * kMaxVerts + 2];
    int2 span[2 * kMaxVerts + 1];
    int ns;
};

// Draw.c's ROUND_UP / ROUND_DOWN: halves go away from / towards the span, on |f| for negative f
__device__ __forceinline__ int round_up_px(float f) { return f >= 0.0f ? (int)floorf(f + 0.5f) : -(int)floorf(fabsf(f) + 0.5f); }
__device__ __forceinline__ int round_down_px(float f) { return f >= 0.0f ? (int)ceilf(f - 0.5f) : -(int)ceilf(fabsf(f) - 0.5f); }

struct Edge {
    int x0, y0, x1, y1;
    __device__ int lo() const { return y0 < y1 ? y0 : y1; }
    __device__ int hi() const { return y0 < y1 ? y1 : y0; }
    __device__ int vertex_x(int y) const { return y == y0 ? x0 : x1; }  // of the end that lies on row y
    __device__ float dx() const { return (float)(x1 - x0) / (float)(y1 - y0); }
    __device__ float at(int y) const { return (float)(y - y0) * dx() + (float)x0; }  // two roundings, as in PIL's C: the pragma above keeps them apart
};
__device__ __forceinline__ Edge edge_of(const int2* v, int n, int e) {
    const int2 a = v[e], b = v[e + 1 == n ? 0 : e + 1];
    return Edge{a.x, a.y, b.x, b.y};
}

// The spans PIL fills on row y of an H-row canvas (x unclipped), by one lane.
__device__ void row_spans(RowScratch& s, int n, int H, int y) {
    int ns = 0;
    // the edge list of ImagingDrawPolygon: vertex i -> i + 1, and the closing edge unless the last vertex repeats the first
    const int ne = n < 2 ? 0 : (n - 1) + ((s.v[n - 1].x != s.v[0].x || s.v[n - 1].y != s.v[0].y) ? 1 : 0);
    int pymin = H - 1, pymax = 0;
    for (int e = 0; e < ne; ++e) {
        const Edge ed = edge_of(s.v, n, e);
        pymin = min(pymin, ed.lo());
        pymax = max(pymax, ed.hi());
        if (ed.y0 == ed.y1 && ed.y0 == y) s.span[ns++] = make_int2(min(ed.x0, ed.x1), max(ed.x0, ed.x1));  // a horizontal edge is its own hline
    }
    pymin = max(pymin, 0);
    pymax = min(pymax, H);  // (H, not H - 1: the rows are clipped later, the comparisons below see H)
    if (y >= pymin && y <= pymax) {
        int j = 0;
        for (int i = 0; i < ne; ++i) {
            const Edge cur = edge_of(s.v, n, i);
            if (cur.y0 == cur.y1 || y < cur.lo() || y > cur.hi()) continue;
            const float cdx = cur.dx(), x = cur.at(y);
            s.xx[j++] = x;
            if (y == cur.hi() && y < pymax) {  // an edge ending on an inner row counts twice
                s.xx[j++] = x;
            } else if (cdx != 0.0f && (y == cur.y0 || y == cur.y1)) {
                // a corner: this edge and an earlier one leaning the same way share the vertex on this row (the integer vertex decides: the
                // fp32 crossing of an edge at its far end is rounded).  Its row is extended towards the span of the next row (the previous
                // one on the last row), up to the pixel beside it
                const int apex = cur.vertex_x(y);
                for (int k = 0; k < i; ++k) {
                    const Edge oth = edge_of(s.v, n, k);
                    if (oth.y0 == oth.y1) continue;
                    const float odx = oth.dx();
                    if ((cdx > 0.0f && odx <= 0.0f) || (cdx < 0.0f && odx >= 0.0f)) continue;
                    if (!((y == cur.lo() && y == oth.lo()) || (y == cur.hi() && y == oth.hi()))) continue;
                    if (oth.vertex_x(y) != apex) continue;
                    const int off = y == pymax ? -1 : 1;
                    const float a = cur.at(y + off), b = oth.at(y + off);
                    int px;
                    if ((cdx > 0.0f) == (off == 1))
                        px = max(apex, round_up_px(fminf(a, b)) - 1);
                    else
                        px = min(apex, round_up_px(fmaxf(a, b) + 1.0f));
                    s.xx[j - 1] = (float)px;
                    break;
                }
            }
        }
        for (int a = 1; a < j; ++a) {  // insertion sort: a handful of crossings
            const float key = s.xx[a];
            int b = a - 1;
            while (b >= 0 && s.xx[b] > key) {
                s.xx[b + 1] = s.xx[b];
                --b;
            }
            s.xx[b + 1] = key;
        }
        int x_pos = j ? (int)s.xx[0] : 0;
        for (int i = 1; i < j; i += 2) {
            const int x_end = round_down_px(s.xx[i]);
            if (x_end < x_pos) continue;
            int x_start = round_up_px(s.xx[i - 1]);
            if (x_pos > x_start) {
                x_start = x_pos;
                if (x_end < x_start) continue;
            }
            s.span[ns++] = make_int2(x_start, x_end);
            x_pos = x_end + 1;
        }
    }
    s.ns = ns;
}

// Row y of one polygon's (H, W) mask into row[0 .. W); the whole workgroup (64 lanes) calls this.
__device__ void mask_row(RowScratch& s, const int* __restrict__ verts, int n, int H, int W, int y, uint8_t* __restrict__ row) {
    const int t = threadIdx.x;
    n = n < 0 ? 0 : (n > kMaxVerts ? kMaxVerts : n);
    for (int i = t; i < n; i += 64) s.v[i] = make_int2(verts[2 * i], verts[2 * i + 1]);
    for (int x = t; x < W; x += 64) row[x] = 0;
    __syncthreads();
    if (t == 0) row_spans(s, n, H, y);
    __syncthreads();
    for (int k = 0; k < s.ns; ++k) {
        const int lo = max(s.span[k].x, 0), hi = min(s.span[k].y, W - 1);
        for (int x = lo + t; x <= hi; x += 64) row[x] = 1;
    }
}

__global__ __launch_bounds__(64) void k_line_mask(const int* __restrict__ verts, const long long* __restrict__ vert_offs,
                                                  const int* __restrict__ vert_counts, const int* __restrict__ sizes,
                                                  const long long* __restrict__ out_offs, uint8_t* __restrict__ out) {
    __shared__ RowScratch s;
    const int b = blockIdx.y, y = blockIdx.x;
    const int H = sizes[2 * b], W = sizes[2 * b + 1];
    if (y >= H) return;
    mask_row(s, verts + 2 * vert_offs[b], vert_counts[b], H, W, y, out + out_offs[b] + (long long)y * W);
}

// batch_offs [B][3]: the offsets ocrs_augment_lines takes; element 0 = where the sample's crop (and mask) starts in the packed batch
__global__ __launch_bounds__(64) void k_line_batch(const uint8_t* __restrict__ pixels, const long long* __restrict__ px_offs,
                                                   const int* __restrict__ sizes, const int* __restrict__ verts,
                                                   const long long* __restrict__ vert_offs, const int* __restrict__ vert_counts, int N,
                                                   const int* __restrict__ indices, const long long* __restrict__ batch_offs,
                                                   uint8_t* __restrict__ crops, uint8_t* __restrict__ masks) {
    __shared__ RowScratch s;
    const int b = blockIdx.y, y = blockIdx.x;
    int l = indices[b];
    l = l < 0 ? 0 : (l >= N ? N - 1 : l);  // (indices are checked on the host; never read outside the store)
    const int H = sizes[2 * l], W = sizes[2 * l + 1];
    if (y >= H) return;
    const long long at = batch_offs[3 * b] + (long long)y * W;
    const uint8_t* src = pixels + px_offs[l] + (long long)y * W;
    uint8_t* dst = crops + at;
    if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {  // 16 bytes per lane where the row allows it
        const int nv = W >> 4;
        for (int i = threadIdx.x; i < nv; i += 64) reinterpret_cast<uint4*>(dst)[i] = reinterpret_cast<const uint4*>(src)[i];
        for (int x = (nv << 4) + threadIdx.x; x < W; x += 64) dst[x] = src[x];
    } else {
        for (int x = threadIdx.x; x < W; x += 64) dst[x] = src[x];
    }
    mask_row(s, verts + 2 * vert_offs[l], vert_counts[l], H, W, y, masks + at);
}

}  // namespace

extern "C" {

int ocrs_line_mask(const int* vertices, const long long* vertex_offs, const int* vertex_counts, const int* sizes, const long long* out_offs,
                   void* out_u8, int n, int max_h, hipStream_t st) {
    OCRS_CHECK_ARG(n >= 0 && n <= 65535);
    if (n == 0) return OCRS_OK;
    OCRS_CHECK_ARG(vertices && vertex_offs && vertex_counts && sizes && out_offs && out_u8 && max_h >= 1 && max_h <= 65535);
    hipLaunchKernelGGL(k_line_mask, dim3(max_h, n), dim3(64), 0, st, vertices, vertex_offs, vertex_counts, sizes, out_offs,
                       static_cast<uint8_t*>(out_u8));
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

int ocrs_line_batch(const void* pixels_u8, const long long* pixel_offs, const int* sizes, const int* vertices, const long long* vertex_offs,
                    const int* vertex_counts, int N, const int* indices, int B, int max_h, const long long* batch_offs, void* out_crops_u8,
                    void* out_masks_u8, hipStream_t st) {
    OCRS_CHECK_ARG(B >= 0 && B <= 65535 && N >= 1);
    if (B == 0) return OCRS_OK;
    OCRS_CHECK_ARG(pixels_u8 && pixel_offs && sizes && vertices && vertex_offs && vertex_counts && indices && batch_offs && out_crops_u8 &&
                   out_masks_u8 && max_h >= 1 && max_h <= 65535);
    hipLaunchKernelGGL(k_line_batch, dim3(max_h, B), dim3(64), 0, st, static_cast<const uint8_t*>(pixels_u8), pixel_offs, sizes, vertices,
                       vertex_offs, vertex_counts, N, indices, batch_offs, static_cast<uint8_t*>(out_crops_u8),
                       static_cast<uint8_t*>(out_masks_u8));
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

}  // extern "C"
