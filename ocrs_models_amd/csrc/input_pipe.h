// Device helpers shared by the input pipeline (input_pipe.hip) and the training augmentations (augment.hip), so both compute the same
// bits: the uint8 -> [-0.5, 0.5] map of transform_image and ATen's antialiased-resize weight rule.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ float px_u8(unsigned v) { return (float)v / 255.0f - 0.5f; }  // IEEE fp32 divide, same value as ATen's

// ---- antialiased bilinear resize: one pass per axis, one thread per output element ------------------------------------------
// ATen's weights for output index i along an axis of input size n, output size m (align_corners = False):
//   scale = n / m; support = max(scale, 1); center = scale * (i + 0.5); lo = max(int(center - support + 0.5), 0);
//   cnt = min(int(center + support + 0.5), n) - lo; w_j = tri((j + lo - center + 0.5) / max(scale, 1)), normalised to sum 1.
struct AaSpan {
    int lo, cnt;
    float center, inv, total;
};
__device__ __forceinline__ AaSpan aa_span(int i, int n, float scale) {
    AaSpan s;
    const float support = scale >= 1.0f ? scale : 1.0f;
    s.inv = scale >= 1.0f ? 1.0f / scale : 1.0f;
    s.center = scale * ((float)i + 0.5f);
    s.lo = max((int)(s.center - support + 0.5f), 0);
    s.cnt = min((int)(s.center + support + 0.5f), n) - s.lo;
    s.total = 0.0f;
    for (int j = 0; j < s.cnt; ++j) s.total += fmaxf(0.0f, 1.0f - fabsf(((float)(j + s.lo) - s.center + 0.5f) * s.inv));
    return s;
}
__device__ __forceinline__ float aa_w(const AaSpan& s, int j) {
    const float w = fmaxf(0.0f, 1.0f - fabsf(((float)(j + s.lo) - s.center + 0.5f) * s.inv));
    return s.total != 0.0f ? w / s.total : w;
}
// one output element of a pass: the span's weights against cnt inputs `stride` elements apart, src at the span's first input.  Every
// antialiased resize (ocrs_resize_aa, ocrs_resize_aa_packed, ocrs_tile_batch) sums through this one loop, which is what makes their results
// the same bits.  A uint8 source is a raw page: every tap goes through px_u8 first, the value transform_image would have stored for it.
__device__ __forceinline__ float aa_tap(const float* p) { return *p; }
__device__ __forceinline__ float aa_tap(const uint8_t* p) { return px_u8(*p); }
template <typename S>
__device__ __forceinline__ float aa_dot(const AaSpan& s, const S* __restrict__ src, size_t stride) {
    float acc = 0.0f;
    for (int j = 0; j < s.cnt; ++j) acc += aa_w(s, j) * aa_tap(src + (size_t)j * stride);
    return acc;
}

}  // namespace
