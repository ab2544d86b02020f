// Page orientation (DESIGN.md §22 states the convention and the rule; the numpy restatement is tests/orient_ref.py; Python:
// inference/orient.py): a page scanned sideways or upside down is turned upright by a multiple of 90 degrees -- an exact permutation of its
// bytes -- before the pipeline runs, and the geometry of the result is mapped back.  orientation = k means upright = rot90(page, k), k
// quarter turns counter-clockwise.
//
//   k_turn_quarter<K, Wide>  k = 1, 3: a 64 x 64 byte tile through LDS.  Wide (H, W multiples of 4, 4-byte aligned bases): every lane loads
//                            one dword of a source row and, after the barrier, reads a 4 x 4 byte block as four dwords, transposes it in
//                            registers and stores one dword to each of four destination rows; both sides move 64 contiguous bytes per row
//                            and 16 lanes.  The tile's pitch is 17 dwords, so the block reads of a half wave -- 8 row groups x 4 dword
//                            columns -- fall on 32 different banks.  Otherwise the same tile moves byte by byte with every index checked.
//   k_turn_half              k = 2: dst[n - 1 - e] = src[e]; a lane loads 16 source bytes, reverses them in registers (byte swap of each
//                            dword, dwords in reverse order) and stores them as one aligned 16-byte piece; the ragged ends go bytewise.
//   k_turn_quads             the point table of the convention, or its inverse, on (N,4,2) fp32 quads: one fp32 subtraction or a copy per
//                            coordinate.
//   k_orient_votes           one workgroup: the long side of every quad by the crop-frame rule, the voters' lengths summed by direction.
//                            Lane t adds quads t, t + 1024, ... in index order in fp64, then one fixed shuffle tree and one fixed chain
//                            over the 16 waves: no atomics, equal input gives equal bytes.
//   k_orient_picks           the voters ranked by length (ties: the smaller index first) by counting, 256 candidates per workgroup against
//                            tiles of 256 lengths staged in LDS; rank r < sample writes picks[r].
//   k_path_confidence        one wave per crop: per time step the maximum over the classes (lanes across the classes, exact), summed in
//                            time order in fp64 by every lane alike, divided by the number of steps.
//
// Lengths are sqrtf(ex * ex + ey * ey) with one rounding per operation (no fused multiply-add), so the restatement follows them bit by bit.
#include "common.h"

#pragma clang fp contract(off)
#include "crop_frame.h"  // (behind the pragma: long_side() is compiled here with one rounding per operation)

namespace {

constexpr int kTile = 64;             // bytes per tile side
constexpr int kPitch = kTile / 4 + 1;  // dwords per tile row in LDS

// ---- the turn ----------------------------------------------------------------------------------------------------------------------------
// byte q of each of four dwords -> one dword, a[0]'s byte lowest
__device__ __forceinline__ unsigned column_of(const unsigned (&a)[4], int q) {
    return ((a[0] >> (8 * q)) & 0xffu) | (((a[1] >> (8 * q)) & 0xffu) << 8) | (((a[2] >> (8 * q)) & 0xffu) << 16) | (((a[3] >> (8 * q)) & 0xffu) << 24);
}

// src (H,W) -> dst (W,H).  K = 1: dst[W - 1 - c][r] = src[r][c];  K = 3: dst[c][H - 1 - r] = src[r][c].
template <int K, bool Wide>
__global__ __launch_bounds__(256) void k_turn_quarter(const uint8_t* __restrict__ src, int H, int W, uint8_t* __restrict__ dst) {
    __shared__ unsigned s_tile[kTile * kPitch];
    const long r0 = (long)blockIdx.y * kTile, c0 = (long)blockIdx.x * kTile;
    {
        const int cd = threadIdx.x & 15, rr = threadIdx.x >> 4;  // dword column, row within a group of 16
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long r = r0 + rr + 16 * i, c = c0 + 4 * cd;
            unsigned v = 0;
            if constexpr (Wide) {
                if (r < H && c < W) v = *reinterpret_cast<const unsigned*>(src + r * W + c);
            } else {
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if (r < H && c + b < W) v |= (unsigned)src[r * W + c + b] << (8 * b);
            }
            s_tile[(rr + 16 * i) * kPitch + cd] = v;
        }
    }
    __syncthreads();
    // this lane's 4 x 4 block: rows 4 rb .. 4 rb + 3, dword column cb.  A half wave holds rb in 0..7 (or 8..15) and four cb: banks
    // (4 rb * 17 + cb) mod 32 = 4 rb + cb, all different.
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rb = (lane & 7) | ((lane >> 5) << 3), cb = ((lane >> 3) & 3) + 4 * wave;
    unsigned a[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = s_tile[(4 * rb + i) * kPitch + cb];
    if (K == 3) {  // the destination row runs against the source rows
        unsigned t = a[0];
        a[0] = a[3], a[3] = t;
        t = a[1], a[1] = a[2], a[2] = t;
    }
    const long r = r0 + 4 * rb, c = c0 + 4 * cb;
    const long j0 = K == 1 ? r : (long)H - 4 - r;  // first destination column of the block (may be < 0 at a ragged edge)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const unsigned v = column_of(a, q);
        const long i = K == 1 ? (long)W - 1 - (c + q) : c + q;  // destination row
        if (c + q >= W) continue;
        if constexpr (Wide) {
            if (r < H) *reinterpret_cast<unsigned*>(dst + i * H + j0) = v;
        } else {
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const long j = j0 + b;
                if (j >= 0 && j < H && (K == 1 ? r + b : r + 3 - b) < H) dst[i * H + j] = (uint8_t)(v >> (8 * b));
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_turn_half(const uint8_t* __restrict__ src, long n, uint8_t* __restrict__ dst, int dst_aligned) {
    const long d0 = ((long)blockIdx.x * 256 + threadIdx.x) * 16;  // destination bytes d0 .. d0 + 15 = source bytes n - 1 - d0 down to n - 16 - d0
    if (d0 >= n) return;
    if (d0 + 16 <= n) {
        uint4 v;
        __builtin_memcpy(&v, src + (n - 16 - d0), 16);  // (any alignment: the compiler picks the loads)
        const uint4 o = make_uint4(__builtin_bswap32(v.w), __builtin_bswap32(v.z), __builtin_bswap32(v.y), __builtin_bswap32(v.x));
        if (dst_aligned)
            *reinterpret_cast<uint4*>(dst + d0) = o;
        else
            __builtin_memcpy(dst + d0, &o, 16);
    } else {
        for (long d = d0; d < n; ++d) dst[d] = src[n - 1 - d];
    }
}

// ---- quads ---------------------------------------------------------------------------------------------------------------------------------
// one lane = one point.  wm = W - 1, hm = H - 1 as fp32 (exact: both below 2^24).
__global__ __launch_bounds__(256) void k_turn_quads(const float* __restrict__ quads, long n, const int* __restrict__ count, float wm, float hm, int k, int inverse,
                                                    float* __restrict__ out) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= 4 * row_count(count, n)) return;
    const float2 in = reinterpret_cast<const float2*>(quads)[p];
    float2 o = in;
    if (k == 2) o = make_float2(wm - in.x, hm - in.y);
    if (k == 1) o = inverse ? make_float2(in.y, wm - in.x) : make_float2(wm - in.y, in.x);
    if (k == 3) o = inverse ? make_float2(hm - in.y, in.x) : make_float2(in.y, hm - in.x);
    reinterpret_cast<float2*>(out)[p] = o;
}

// ---- votes -----------------------------------------------------------------------------------------------------------------------------------
// The long side of a quad by the crop-frame rule (csrc/crop_frame.h: the longer of c0->c1 and c1->c2; on a tie the one with the larger |x|).
// -> its length if the quad votes (short > 0 and long >= min_aspect * short), else -1; horiz: |L.x| >= |L.y|.
__device__ __forceinline__ float vote_length(const float* __restrict__ q, float min_aspect, bool& horiz) {
    const LongSide s = long_side(reinterpret_cast<const float4*>(q)[0], reinterpret_cast<const float4*>(q)[1]);
    horiz = fabsf(s.x) >= fabsf(s.y);
    return (s.sht > 0.0f && s.lng >= min_aspect * s.sht) ? s.lng : -1.0f;  // (a NaN length fails both comparisons)
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// votes: 2 fp64 (H, V) then 2 int32 (voters, K = min(sample, voters)); picks [sample] is set to -1 for k_orient_picks to fill.
__global__ __launch_bounds__(1024) void k_orient_votes(const float* __restrict__ quads, long n, const int* __restrict__ count, float min_aspect, int sample,
                                                       double* __restrict__ votes, int* __restrict__ picks) {
    __shared__ double s_h[16], s_v[16];
    __shared__ int s_n[16];
    const long m = row_count(count, n);
    for (int t = threadIdx.x; t < sample; t += 1024) picks[t] = -1;
    double h = 0.0, v = 0.0;
    int voters = 0;
    for (long i = threadIdx.x; i < m; i += 1024) {
        bool horiz;
        const float len = vote_length(quads + i * 8, min_aspect, horiz);
        if (len >= 0.0f) {
            ++voters;
            if (horiz)
                h += (double)len;
            else
                v += (double)len;
        }
    }
    h = wave_sum_f64(h), v = wave_sum_f64(v);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) voters += __shfl_xor(voters, o, 64);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) s_h[wave] = h, s_v[wave] = v, s_n[wave] = voters;
    __syncthreads();
    if (threadIdx.x == 0) {
        double th = 0.0, tv = 0.0;
        int tn = 0;
        for (int w = 0; w < 16; ++w) th += s_h[w], tv += s_v[w], tn += s_n[w];
        votes[0] = th, votes[1] = tv;
        int* counts = reinterpret_cast<int*>(votes + 2);
        counts[0] = tn, counts[1] = min(sample, tn);
    }
}

__global__ __launch_bounds__(256) void k_orient_picks(const float* __restrict__ quads, long n, const int* __restrict__ count, float min_aspect, int sample,
                                                      int* __restrict__ picks) {
    __shared__ float s_len[256];
    const long m = row_count(count, n);
    if ((long)blockIdx.x * 256 >= m) return;  // (workgroup-uniform)
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    bool horiz;
    const float mine = i < m ? vote_length(quads + i * 8, min_aspect, horiz) : -1.0f;
    long rank = 0;
    for (long base = 0; base < m; base += 256) {
        const long j = base + threadIdx.x;
        __syncthreads();
        s_len[threadIdx.x] = j < m ? vote_length(quads + j * 8, min_aspect, horiz) : -1.0f;
        __syncthreads();
        const int cnt = (int)min(256L, m - base);
        for (int t = 0; t < cnt; ++t) {
            const float other = s_len[t];  // (one address for the whole wave: a broadcast read)
            rank += (other > mine || (other == mine && base + t < i)) ? 1 : 0;
        }
    }
    if (mine >= 0.0f && rank < sample) picks[rank] = (int)i;  // non-voters hold -1 and never outrank a voter
}

// ---- path confidence ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_path_confidence(const float* __restrict__ lp, int T, int B, int C, const int* __restrict__ steps, double* __restrict__ scores) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= B) return;  // (wave-uniform; the kernel has no barrier)
    const int n = min(max(steps[r], 0), T);
    double sum = 0.0;
    for (int t = 0; t < n; ++t) {
        const float* row = lp + ((long)t * B + r) * C;
        float m = -INFINITY;
        for (int c = lane; c < C; c += 64) m = fmaxf(m, row[c]);
        sum += (double)wave_max(m);  // every lane holds the same maximum and adds it in the same order
    }
    if (lane == 0) scores[r] = n > 0 ? sum / (double)n : 0.0;
}

}  // namespace

extern "C" {

int ocrs_turn_page_u8(const unsigned char* src, int H, int W, int k, unsigned char* dst, hipStream_t st) {
    OCRS_CHECK_ARG(H >= 1 && W >= 1 && k >= 1 && k <= 3 && src && dst && src != dst);
    OCRS_CHECK_ARG((H + kTile - 1) / kTile <= 65535 && (W + kTile - 1) / kTile <= 65535);
    const long n = (long)H * W;
    if (k == 2) {
        const long blocks = (n + 4095) / 4096;
        OCRS_CHECK_ARG(blocks < (1L << 31));
        hipLaunchKernelGGL(k_turn_half, dim3((unsigned)blocks), dim3(256), 0, st, src, n, dst, (int)aligned16(dst));
    } else {
        const dim3 grid((unsigned)((W + kTile - 1) / kTile), (unsigned)((H + kTile - 1) / kTile));
        const bool wide = H % 4 == 0 && W % 4 == 0 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 3) == 0;
        if (k == 1 && wide) hipLaunchKernelGGL((k_turn_quarter<1, true>), grid, dim3(256), 0, st, src, H, W, dst);
        if (k == 1 && !wide) hipLaunchKernelGGL((k_turn_quarter<1, false>), grid, dim3(256), 0, st, src, H, W, dst);
        if (k == 3 && wide) hipLaunchKernelGGL((k_turn_quarter<3, true>), grid, dim3(256), 0, st, src, H, W, dst);
        if (k == 3 && !wide) hipLaunchKernelGGL((k_turn_quarter<3, false>), grid, dim3(256), 0, st, src, H, W, dst);
    }
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

int ocrs_turn_quads(const float* quads, long n, const int* count, int H, int W, int k, int inverse, float* out, hipStream_t st) {
    OCRS_CHECK_ARG(n >= 0 && n < (1L << 29) && H >= 1 && W >= 1 && H <= (1 << 24) && W <= (1 << 24) && k >= 0 && k <= 3);
    if (n == 0) return OCRS_OK;
    OCRS_CHECK_ARG(quads && out && (reinterpret_cast<uintptr_t>(quads) & 7) == 0 && (reinterpret_cast<uintptr_t>(out) & 7) == 0);
    hipLaunchKernelGGL(k_turn_quads, dim3((unsigned)((4 * n + 255) / 256)), dim3(256), 0, st, quads, n, count, (float)(W - 1), (float)(H - 1), k, inverse != 0, out);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

int ocrs_orient_votes(const float* quads, long n, const int* count, float min_aspect, int sample, double* votes, int* picks, hipStream_t st) {
    OCRS_CHECK_ARG(n >= 0 && n < (1L << 29) && sample >= 0 && votes && (reinterpret_cast<uintptr_t>(votes) & 7) == 0 && (sample == 0 || picks));
    OCRS_CHECK_ARG(n == 0 || (quads && aligned16(quads)));
    hipLaunchKernelGGL(k_orient_votes, dim3(1), dim3(1024), 0, st, quads, n, count, min_aspect, sample, votes, picks);
    if (n > 0 && sample > 0)
        hipLaunchKernelGGL(k_orient_picks, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, quads, n, count, min_aspect, sample, picks);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

int ocrs_path_confidence(const float* log_probs, int T, int B, int C, const int* steps, double* scores, hipStream_t st) {
    OCRS_CHECK_ARG(T >= 1 && B >= 0 && C >= 1);
    if (B == 0) return OCRS_OK;
    OCRS_CHECK_ARG(log_probs && steps && scores && (reinterpret_cast<uintptr_t>(scores) & 7) == 0);
    hipLaunchKernelGGL(k_path_confidence, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, log_probs, T, B, C, steps, scores);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

}  // extern "C"
