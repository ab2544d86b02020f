// One-wave Levenshtein distance, shared by the recognition loops' character error rate (rec_cer.hip, whose header comment describes the sweep)
// and the end-to-end accuracy of page OCR (ocr_eval.hip).  Integers only: every result is exact.
#pragma once
#include "common.h"

namespace {

constexpr int DPP_WAVE_SHR1 = 0x138;  // result[i] = src[i - 1]; lane 0 has no source and keeps `old`
__device__ __forceinline__ int wave_shr1(int lane0, int v) { return __builtin_amdgcn_update_dpp(lane0, v, DPP_WAVE_SHR1, 0xF, 0xF, false); }

// The host compares characters, not class ids (an alphabet with a repeated character makes two ids equal): ids inside the table are mapped
// through it, anything else compares as itself.
__device__ __forceinline__ int code_of(const int* __restrict__ codes, int ncodes, int x) {
    return (codes && (unsigned)x < (unsigned)ncodes) ? codes[x] : x;
}

// Levenshtein distance (unit costs) of a[0..m) and b[0..n) by the calling wave; all 64 lanes must be active, m and n wave-uniform.
// bnd: m ints of scratch for the boundary column between passes (only touched when n > 64).  Every lane returns the distance.
__device__ int wave_edit_distance(const int* a, int m, const int* b, int n, const int* __restrict__ codes, int ncodes, int* bnd, int lane) {
    if (m == 0 || n == 0) return m + n;
    const int npass = (n + 63) >> 6;
    int result = 0;
    for (int p = 0; p < npass; ++p) {
        const int c0 = p * 64, col = c0 + lane;
        const bool last = p == npass - 1;
        const int jlast = last ? n - 1 - c0 : 63;  // last lane with a column of b in this pass
        const int bj = col < n ? code_of(codes, ncodes, b[col]) : -1;  // (lanes beyond n compute values nobody reads)
        const int steps = m + jlast;
        int cur = col + 1;  // D[0][col + 1]
        int diag = col;     // D[0][col]: what the shift delivers while the lane below has not started
        int ch = 0;
        // 64-step chunks: lane k of a_cur / b_cur holds a's label and the boundary value D[r][c0] of row r = d0 + k + 1 (the row index itself
        // in pass 0, bnd[r - 1] otherwise); the next chunk is in flight while this one is swept
        int a_nxt = lane < m ? code_of(codes, ncodes, a[lane]) : 0;
        int b_nxt = p == 0 ? lane + 1 : (lane < m ? bnd[lane] : 0);
        for (int d0 = 0; d0 < steps; d0 += 64) {
            const int a_cur = a_nxt, b_cur = b_nxt;
            const int r = d0 + 64 + lane;  // the prefetched rows lie 64 or more ahead of the rows this chunk's boundary store overwrites
            a_nxt = r < m ? code_of(codes, ncodes, a[r]) : 0;
            b_nxt = p == 0 ? r + 1 : (r < m ? bnd[r] : 0);
            const int kend = min(64, steps - d0);
            int out = 0;  // lane k: lane 63's value after step d0 + k = D[d0 + k - 62][c0 + 64]
            for (int k = 0; k < kend; ++k) {
                ch = wave_shr1(__builtin_amdgcn_readlane(a_cur, k), ch);
                const int left = wave_shr1(__builtin_amdgcn_readlane(b_cur, k), cur);
                const int v = min(min(cur, left) + 1, diag + (ch != bj ? 1 : 0));
                cur = (unsigned)(d0 + k - lane) < (unsigned)m ? v : cur;  // row d0 + k - lane of a; outside [0, m) the lane idles
                diag = left;
                if (!last) out = lane == k ? __builtin_amdgcn_readlane(cur, 63) : out;
            }
            const int row = d0 + lane - 63;
            if (!last && lane < kend && (unsigned)row < (unsigned)m) bnd[row] = out;
        }
        if (last) result = __builtin_amdgcn_readlane(cur, jlast);
        __syncthreads();  // (one-wave block) lane 63's boundary stores are visible to the chunk loads of the next pass
    }
    return result;
}

}  // namespace
