// Text in mixed directions on one page (DESIGN.md §24 states the rule; the numpy restatement is tests/directions_ref.py; Python:
// inference/directions.py): the sideways words of a page are read as the words of a second, virtual page -- the page turned by one quarter
// turn -- through the page-batch path, and a recogniser probe decides per sideways line which way up it reads.
//
//   k_axis_split     classifies every word quad by the direction of its long side (the crop-frame rule), compacts the upright words in
//                    front of the sideways ones, both in input order, and maps the sideways ones to the turned page in the same pass.
//                    One workgroup per 256 words and no workspace: every workgroup counts the sideways words in front of its own 256 (and
//                    on the whole page) by classifying them again -- N is a few thousand, the quads sit in L2 -- then one block_scan_256
//                    over its own words gives every lane its row.  No atomic counter: the order does not depend on which workgroup
//                    arrives first.  A lane loads and stores its quad as two 16-byte pieces.
//   k_flip_crops     one lane = four consecutive floats of one row of the OUTPUT batch.  Wide (Wpad a multiple of 4, 16-byte aligned
//                    output): a piece inside a flagged crop's valid width loads its four source floats -- they end at column w - 1 - d0 of
//                    the opposite row, so their address is 4-byte aligned only -- reverses them in registers and stores one aligned 16-byte
//                    piece; a piece outside it is a 16-byte copy; the one piece that straddles w goes element by element.  The 64 loads
//                    of a wave cover one contiguous span of the source row (read backwards), so no staging through LDS is needed for
//                    either side to move whole lines.  Otherwise every element is moved on its own with its index checked.
//   k_flip_flags     the strict fp64 comparison of the two probe scores, masked by the crop's page.
#include "common.h"

#pragma clang fp contract(off)
#include "crop_frame.h"  // (behind the pragma: long_side() is compiled here with one rounding per operation)

namespace {

// a = (x0, y0, x1, y1), c = (x2, y2, x3, y3).  The long side is crop_frame.h's, the one the crop frame and k_orient_votes use.
__device__ __forceinline__ int sideways(const float4 a, const float4 c) {
    const LongSide s = long_side(a, c);
    const bool numbers = a.x == a.x && a.y == a.y && a.z == a.z && a.w == a.w && c.x == c.x && c.y == c.y && c.z == c.z && c.w == c.w;
    return (numbers && fabsf(s.y) > fabsf(s.x)) ? 1 : 0;  // exactly 45 degrees is upright
}

__device__ __forceinline__ int sideways_row(const float* __restrict__ quads, long i) {
    const float4* q = reinterpret_cast<const float4*>(quads + i * 8);
    return sideways(q[0], q[1]);
}

// wm = W - 1 as fp32 (exact: below 2^24)
__global__ __launch_bounds__(256) void k_axis_split(const float* __restrict__ quads, long n, const int* __restrict__ count, float wm, float* __restrict__ out,
                                                    int* __restrict__ page_of_word, int* __restrict__ word_offs, int* __restrict__ source_index) {
    __shared__ int s_before[4], s_total[4];
    const int m = (int)row_count(count, n);
    const int t = threadIdx.x, first = (int)blockIdx.x * 256;
    if (first >= m && blockIdx.x != 0) return;  // (workgroup-uniform; workgroup 0 stays to write word_offs)
    int before = 0, total = 0;  // sideways words in front of this workgroup's rows, and among all m
    for (int i = t; i < m; i += 256) {
        const int s = sideways_row(quads, i);
        total += s;
        before += i < first ? s : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o, 64), total += __shfl_xor(total, o, 64);
    if ((t & 63) == 0) s_before[t >> 6] = before, s_total[t >> 6] = total;
    __syncthreads();
    before = (s_before[0] + s_before[1]) + (s_before[2] + s_before[3]);
    total = (s_total[0] + s_total[1]) + (s_total[2] + s_total[3]);
    const int i = first + t;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), c = a;
    if (i < m) a = reinterpret_cast<const float4*>(quads + (long)i * 8)[0], c = reinterpret_cast<const float4*>(quads + (long)i * 8)[1];
    const int s = i < m ? sideways(a, c) : 0;
    const int2 sc = block_scan_256(s);
    if (i < m) {
        const int rank = before + sc.x - s;                      // sideways words in front of word i
        const int row = s ? (m - total) + rank : i - rank;       // 0 <= row < m: the upright words fill rows 0 .. m - total - 1
        if (s) a = make_float4(a.y, wm - a.x, a.w, wm - a.z), c = make_float4(c.y, wm - c.x, c.w, wm - c.z);
        reinterpret_cast<float4*>(out + (long)row * 8)[0] = a;
        reinterpret_cast<float4*>(out + (long)row * 8)[1] = c;
        page_of_word[row] = s;
        source_index[row] = i;
    }
    if (blockIdx.x == 0 && t == 0) word_offs[0] = 0, word_offs[1] = m - total, word_offs[2] = m;
}

// pieces = n * OH * ppr lanes, ppr = ceil(Wpad / 4) pieces per row.  The batches are moved as 32-bit words: a permutation of bits.
template <bool Wide>
__global__ __launch_bounds__(256) void k_flip_crops(const unsigned* __restrict__ in, unsigned* __restrict__ out, unsigned pieces, unsigned ppr, unsigned OH, int Wpad,
                                                    const long long* __restrict__ widths, const int* __restrict__ flags) {
    const unsigned p = blockIdx.x * 256u + threadIdx.x;
    if (p >= pieces) return;
    const unsigned r = p / ppr, i = r / OH;  // row of the batch, crop
    const unsigned y = r - i * OH;
    const int d0 = 4 * (int)(p - r * ppr);   // first column of the piece
    const int w = (int)min(max(widths[i], 0LL), (long long)Wpad);
    const bool turn = flags ? flags[i] != 0 : true;
    const unsigned* same = in + (long)r * Wpad;                                // row y of crop i
    const unsigned* opposite = in + ((long)i * OH + (OH - 1 - y)) * Wpad;      // row OH - 1 - y
    unsigned* dst = out + (long)r * Wpad;
    if constexpr (Wide) {  // d0 + 4 <= Wpad, dst + d0 is 16-byte aligned
        if (!turn || d0 >= w) {
            uint4 v;
            __builtin_memcpy(&v, same + d0, 16);  // (the input's base may be 4-byte aligned only: the compiler picks the loads)
            *reinterpret_cast<uint4*>(dst + d0) = v;
            return;
        }
        if (d0 + 4 <= w) {  // columns d0 .. d0 + 3 come from columns w - 1 - d0 down to w - 4 - d0 >= 0
            uint4 v;
            __builtin_memcpy(&v, opposite + (w - 4 - d0), 16);
            *reinterpret_cast<uint4*>(dst + d0) = make_uint4(v.w, v.z, v.y, v.x);
            return;
        }
    }
    const int end = min(d0 + 4, Wpad);
    for (int x = d0; x < end; ++x) dst[x] = (turn && x < w) ? opposite[w - 1 - x] : same[x];
}

__global__ __launch_bounds__(256) void k_flip_flags(const double* __restrict__ s_plain, const double* __restrict__ s_flip, const int* __restrict__ probe, long n,
                                                    int* __restrict__ flags) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    flags[i] = (probe[i] != 0 && s_flip[i] > s_plain[i]) ? 1 : 0;  // (a NaN on either side fails the comparison)
}

}  // namespace

extern "C" {

int ocrs_axis_split(const float* quads, long n, const int* count, int H, int W, float* out_quads, int* page_of_word, int* word_offs, int* source_index,
                    hipStream_t st) {
    // every workgroup classifies all rows again (n * n / 256 classifications): sized for the words of a page, and bounded to that
    OCRS_CHECK_ARG(n >= 0 && n <= (1L << 16) && H >= 1 && W >= 1 && H <= (1 << 24) && W <= (1 << 24));
    if (n == 0) return OCRS_OK;
    OCRS_CHECK_ARG(quads && out_quads && page_of_word && word_offs && source_index && quads != out_quads && aligned16(quads) && aligned16(out_quads));
    hipLaunchKernelGGL(k_axis_split, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, quads, n, count, (float)(W - 1), out_quads, page_of_word, word_offs,
                       source_index);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

int ocrs_flip_crops(const float* batch_in, float* batch_out, long n, int OH, int Wpad, const long long* widths, const int* flags, hipStream_t st) {
    OCRS_CHECK_ARG(n >= 0 && OH >= 1 && Wpad >= 1);
    if (n == 0) return OCRS_OK;
    const long ppr = ((long)Wpad + 3) / 4, pieces = n * OH * ppr;
    OCRS_CHECK_ARG(n < (1L << 31) && pieces < (1L << 32) - 256);  // (the kernel counts pieces in 32 bits)
    OCRS_CHECK_ARG(batch_in && batch_out && widths && batch_in != batch_out);
    OCRS_CHECK_ARG(((reinterpret_cast<uintptr_t>(batch_in) | reinterpret_cast<uintptr_t>(batch_out)) & 3) == 0 && (reinterpret_cast<uintptr_t>(widths) & 7) == 0);
    const dim3 grid((unsigned)((pieces + 255) / 256));
    const unsigned* in = reinterpret_cast<const unsigned*>(batch_in);
    unsigned* out = reinterpret_cast<unsigned*>(batch_out);
    if (Wpad % 4 == 0 && aligned16(batch_out))
        hipLaunchKernelGGL((k_flip_crops<true>), grid, dim3(256), 0, st, in, out, (unsigned)pieces, (unsigned)ppr, (unsigned)OH, Wpad, widths, flags);
    else
        hipLaunchKernelGGL((k_flip_crops<false>), grid, dim3(256), 0, st, in, out, (unsigned)pieces, (unsigned)ppr, (unsigned)OH, Wpad, widths, flags);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

int ocrs_flip_flags(const double* s_plain, const double* s_flip, const int* probe, long n, int* flags, hipStream_t st) {
    OCRS_CHECK_ARG(n >= 0 && n < (1L << 31));
    if (n == 0) return OCRS_OK;
    OCRS_CHECK_ARG(s_plain && s_flip && probe && flags && ((reinterpret_cast<uintptr_t>(s_plain) | reinterpret_cast<uintptr_t>(s_flip)) & 7) == 0);
    hipLaunchKernelGGL(k_flip_flags, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, s_plain, s_flip, probe, n, flags);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

}  // extern "C"
