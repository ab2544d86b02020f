// What the crop samplers share (ocr_infer.hip: k_rectify_crops / k_rectify_crops_pages; line_chain.hip: k_rectify_chain / k_rectify_chain_pages):
// the tiling of the packed crops, the search for a tile's crop in the plan, and the one statement of the tap -- border clamp and the
// four-byte bilinear blend of transform_image values.  The samplers differ only in how a sample finds its page position.
#pragma once
#include "input_pipe.h"

namespace {

constexpr int kTileElems = 1024;  // outputs of one sampler workgroup: 256 lanes x one 16-byte store

// the last of the n > 0 crops whose first tile is <= tile
__device__ __forceinline__ long crop_of_tile(const int* __restrict__ plan, long n, long long tile) {
    long lo = 0, hi = n - 1;
    while (lo < hi) {
        const long mid = (lo + hi + 1) >> 1;
        if (plan[mid * 8 + 5] <= tile) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// the value of the (H, W) page at (px, py), pixel-centre coordinates clamped to the page (border padding)
__device__ __forceinline__ float sample_u8(const uint8_t* __restrict__ page, int H, int W, float px, float py) {
    px = fminf(fmaxf(px, 0.0f), (float)(W - 1)), py = fminf(fmaxf(py, 0.0f), (float)(H - 1));
    const int x0 = (int)px, y0 = (int)py;
    const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
    const float fx = px - (float)x0, fy = py - (float)y0;
    const uint8_t* r0 = page + (size_t)y0 * W;
    const uint8_t* r1 = page + (size_t)y1 * W;
    const float a = px_u8(r0[x0]), b = px_u8(r0[x1]), c = px_u8(r1[x0]), d = px_u8(r1[x1]);
    const float top = a + (b - a) * fx, bot = c + (d - c) * fx;
    return top + (bot - top) * fy;
}

}  // namespace
