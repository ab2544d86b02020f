// Crop frame: the one statement of the geometry rule (inference.py's docstring, "Crop frame"), used by the crop plan and the sampler
// (ocr_infer.hip) and by the character boxes and word ranges (char_spans.hip), which turn positions along a crop back into page coordinates.
#pragma once
#include "common.h"

struct CropFrame {
    float ox, oy, ux, uy, lng, sht;  // origin corner, unit width axis u (v = (-uy, ux)), side lengths along u and v
    int h, w;
};
// rows or columns of a crop whose side is `len` page pixels long (fmaxf also turns a NaN length into 1)
__device__ __forceinline__ int crop_len(float len) { return (int)fminf(fmaxf(rintf(len), 1.0f), 32768.0f); }
// The long side of a quad, the one statement of "which side is the width axis": a = (x0, y0, x1, y1), c = (x2, y2, x3, y3); the longer of
// c0->c1 and c1->c2, on a tie the one with the larger |x| (the first if that ties too).  Lengths are sqrtf(x * x + y * y); the callers that
// are compared bit by bit with a restatement (page_orient.hip, line_dirs.hip) compile with fp contraction off.
struct LongSide {
    float x, y, lng, sht;  // the long side's vector (unsigned choice: as the corners give it), its length, the other side's length
};
__device__ __forceinline__ LongSide long_side(const float4 a, const float4 c) {
    const float e1x = a.z - a.x, e1y = a.w - a.y, e2x = c.x - a.z, e2y = c.y - a.w;
    const float l1 = sqrtf(e1x * e1x + e1y * e1y), l2 = sqrtf(e2x * e2x + e2y * e2y);
    const bool first = l1 > l2 || (l1 == l2 && fabsf(e1x) >= fabsf(e2x));
    LongSide s;
    s.x = first ? e1x : e2x, s.y = first ? e1y : e2y;
    s.lng = first ? l1 : l2, s.sht = first ? l2 : l1;
    return s;
}
// rows of a quad table: min(*count, n) with an optional device count, else n
__device__ __forceinline__ long row_count(const int* __restrict__ count, long n) { return count ? min((long)max(*count, 0), n) : n; }

__device__ __forceinline__ CropFrame crop_frame(const float* __restrict__ q) {
    const float4 a = reinterpret_cast<const float4*>(q)[0], c = reinterpret_cast<const float4*>(q)[1];
    const float xs[4] = {a.x, a.z, c.x, c.z}, ys[4] = {a.y, a.w, c.y, c.w};
    const LongSide s = long_side(a, c);
    CropFrame f;
    f.lng = s.lng;
    f.sht = s.sht;
    f.ux = 1.0f, f.uy = 0.0f;
    if (f.lng > 0.0f) f.ux = s.x / f.lng, f.uy = s.y / f.lng;
    if (f.ux < 0.0f || (f.ux == 0.0f && f.uy < 0.0f)) f.ux = -f.ux, f.uy = -f.uy;
    // v = (-uy, ux); the origin is the corner that is first along u and along v, i.e. the smallest u + v projection
    const float sx = f.ux - f.uy, sy = f.uy + f.ux;
    int k = 0;
    float best = xs[0] * sx + ys[0] * sy;
#pragma unroll
    for (int j = 1; j < 4; ++j) {
        const float p = xs[j] * sx + ys[j] * sy;
        if (p < best) best = p, k = j;
    }
    f.ox = xs[k], f.oy = ys[k];
    f.w = crop_len(f.lng);
    f.h = crop_len(f.sht);
    return f;
}
