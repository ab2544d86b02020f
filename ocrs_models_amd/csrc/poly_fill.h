// PIL's polygon fill, one row at a time (shared by csrc/line_data.hip and csrc/page_data.hip): generate_mask's
// ImageDraw.polygon(poly, fill="white", outline=None) on a mode "1" image (ocrs_models/datasets/util.py:78-110), restated operation by
// operation (tests/hiertext_ref.py is the host restatement this was ported from).  PIL's fill is a sequential scanline algorithm whose result
// depends on the edge order, so ONE lane builds and sorts a row's crossings, exactly in that order, in a scratch of its own.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxVerts = 512;  // per polygon; the host refuses a longer one (ocrs_models_amd/datasets.py)

template <int N>
struct PolyScratch {
    int2 v[N];
    float xx[2 * N + 2];
    int2 span[2 * N + 1];
    int ns;
};
using RowScratch = PolyScratch<kMaxVerts>;

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
template <int N>
__device__ void row_spans(PolyScratch<N>& s, int n, int H, int y) {
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

}  // namespace
