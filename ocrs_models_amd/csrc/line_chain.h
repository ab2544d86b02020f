// Spine lookup of the chain crops: from a position s along a line's spine and an offset t across it to the page.  The one
// device statement of "segment of s" and "P(s, t)", used by the sampler and by the character boxes of line_chain.hip.
//
// A line of n words has the rows 2 * off .. 2 * (off + n) - 1 of the spine table (off = line_offsets[l]), 8 floats each: start, len, A.x, A.y,
// dir.x, dir.y, 0, 0; even rows are words, odd rows the gaps behind them.  The 2 n - 1 segments are those rows without the last word's all-zero
// gap row.  `rows` below points at the line's first row, read as two float4 per row, in global memory or in LDS.
//
// All arithmetic here is fp32 with one rounding per operation, in the order DESIGN.md §21 writes it.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

namespace {

// The last of the nseg >= 1 segments with start <= s[k], for K positions at once: the K searches are independent, so their loads overlap.  The
// trip count depends on nseg alone (wave-uniform) and every step is a select: no divergence whatever the positions are.  A position below
// every start (only a NaN or a negative s can be) gets segment 0.
template <int K>
__device__ __forceinline__ void spine_segments(const float4* __restrict__ rows, int nseg, const float (&s)[K], int (&seg)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k) seg[k] = 0;
    for (int len = nseg; len > 1;) {  // the answer is in [seg, seg + len)
        const int half = len >> 1;
#pragma unroll
        for (int k = 0; k < K; ++k) seg[k] = rows[2 * (seg[k] + half)].x <= s[k] ? seg[k] + half : seg[k];
        len -= half;
    }
}

// P(s, t) on segment seg (the one spine_segments found for s): A + e dir + t normal with e = s - start.  The normal is v = (-dir.y, dir.x)
// on a word; on a gap it turns from the normal of the word before to that of the word after, m = (1 - f) v_k + f v_{k+1}, normalised.
__device__ __forceinline__ float2 spine_point(const float4* __restrict__ rows, int seg, float s, float t) {
    const float4 a = rows[2 * seg], b = rows[2 * seg + 1];  // start, len, A.x, A.y | dir.x, dir.y, 0, 0
    const float e = s - a.x;
    float nx = -b.y, ny = b.x;
    if (seg & 1) {  // a gap: rows seg - 1 and seg + 1 are the words on its two sides (a line's last row is never a segment)
        const float4 p = rows[2 * (seg - 1) + 1], q = rows[2 * (seg + 1) + 1];
        const float f = a.y == 0.0f ? 0.0f : e / a.y;
        const float g = 1.0f - f;
        const float mx = g * -p.y + f * -q.y, my = g * p.x + f * q.x;
        const float nm = sqrtf(mx * mx + my * my);
        nx = -p.y, ny = p.x;  // (|m| = 0 needs opposite axes, which the sign rule of the crop frame excludes: v_k then)
        if (nm > 0.0f) nx = mx / nm, ny = my / nm;
    }
    return make_float2((a.z + e * b.x) + t * nx, (a.w + e * b.y) + t * ny);
}

}  // namespace
