// A word's range in the characters of its line, shared by k_word_chars (char_spans.hip) and k_word_chars_chain
// (line_chain.hip): the two kernels differ only in where a word's boundaries come from.
#pragma once
#include "common.h"

namespace {

// #{ k < n : centre of character k < b }; the centres 0.5f * (s0 + s1) are non-decreasing in k
__device__ __forceinline__ int chars_below(const float* __restrict__ s0, const float* __restrict__ s1, int n, float b) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (0.5f * (s0[mid] + s1[mid]) < b) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// word w owns the characters first .. end - 1 of its line less the spaces at both ends -> word_chars[w]
__device__ __forceinline__ void store_word_range(const int* __restrict__ lab, int first, int end, int space, int* __restrict__ word_chars, long w) {
    while (first < end && lab[first] == space) ++first;
    while (end > first && lab[end - 1] == space) --end;
    *reinterpret_cast<int2*>(word_chars + 2 * w) = make_int2(first, end);
}

}  // namespace
