// Characters of recognised crops (Python: text.greedy_decode_spans, inference.char_boxes / word_chars; restated for the tests in
// tests/chars_ref.py): what the greedy CTC decode keeps of the log-probs besides the collapsed labels, where that puts every character on
// the page, and which word of a line it lies over.
//
//   k_argmax_peak   k_argmax of rec_seq.hip (same walk, same tie rule: the same class) that also stores the maximum it found
//   k_ctc_spans     one wave per sample, 64 time steps per round: run starts by comparison with the neighbouring lane, output slots by ballot +
//                   prefix popcount, the last step of a run from the next start bit, its peak by a segmented max scan across lanes; the run
//                   that is still open at the end of a round is finished by the round in which it ends
//   k_char_boxes    rule (b): time steps -> extent along the crop -> character quad through the crop frame (crop_frame.h)
//   k_word_chars    rule (c): one wave per line; the words' boundaries and their running maximum as a wave scan over 64 words per round;
//                   every word finds the two ends of its range by bisecting the characters' centres (they are non-decreasing), then trims
//
// Integer and latency work over small arrays: no LDS, no atomics, nothing synchronises; equal input gives equal bytes.
#include "char_range.h"
#include "crop_frame.h"

namespace {

constexpr float NEG_INF = -__builtin_huge_valf();

// ---- arg-max with its value ----------------------------------------------------------------------------------------------------------
// 16 lanes per (t, n) row of lp [T][N][C], first maximum on ties: k_argmax's loop and reduction, so the class is k_argmax's.  The maximum is
// one of the row's values, copied, not computed.  amax, peak [N][T].
__global__ __launch_bounds__(256) void k_argmax_peak(const float* __restrict__ lp, int* __restrict__ amax, float* __restrict__ peak, int T, int N, int C) {
    const int sub = threadIdx.x & 15;
    const long row = (long)blockIdx.x * 16 + (threadIdx.x >> 4);  // row = t*N + n
    if (row >= (long)T * N) return;
    float best = NEG_INF;
    int bi = C;
    for (int c = sub; c < C; c += 16) {
        const float v = lp[row * C + c];
        if (v > best || (v == best && c < bi)) {
            best = v;
            bi = c;
        }
    }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ov > best || (ov == best && oi < bi)) {
            best = ov;
            bi = oi;
        }
    }
    if (sub == 0) {
        const int t = (int)(row / N), n = (int)(row - (long)t * N);
        amax[(long)n * T + t] = bi;
        peak[(long)n * T + t] = best;
    }
}

// fp32 bits <-> a signed integer with the same order, so that a maximum of keys is a bit copy of one of the values
__device__ __forceinline__ int order_key(float v) {
    const int b = __float_as_int(v);
    return b ^ ((b >> 31) & 0x7fffffff);
}
__device__ __forceinline__ float key_value(int k) { return __int_as_float(k ^ ((k >> 31) & 0x7fffffff)); }

// ---- collapse with spans -------------------------------------------------------------------------------------------------------------
// One wave per sample n (four samples per workgroup), lane l of round r holds step t = 64 r + l.  A run takes its output slot, label and first
// step where it starts; its last step and peak are written where it ends: in the same round by its own start lane (the end is the lane before
// the next start bit, or the last step of the sample), or, for the one run that reaches past the round, by lane 0 of the round that ends it,
// from the carry (slot, peak so far).  Row n of the outputs is row row0 + n of the caller's arrays, pitch ld >= T; entries from lens on and
// rows of other samples are not touched.
__global__ __launch_bounds__(256) void k_ctc_spans(const int* __restrict__ amax, const float* __restrict__ amax_lp, const long long* __restrict__ in_len, int T, int N,
                                                   long row0, int ld, int* __restrict__ labels, int* __restrict__ t0, int* __restrict__ t1, float* __restrict__ peak,
                                                   int* __restrict__ lens) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;  // (wave-uniform; the kernel has no barrier)
    const long long il = in_len[n];
    const int Ti = il < 0 ? 0 : (il > T ? T : (int)il);
    const int* am = amax + (long)n * T;
    const float* av = amax_lp + (long)n * T;
    const long out = (row0 + n) * (long)ld;
    const unsigned long long below = (1ULL << lane) - 1ULL;  // the lanes before this one
    int count = 0;                                          // characters emitted by the earlier rounds
    int carry_c = -1, carry_slot = -1, carry_key = 0;       // class of the step before this round; slot and peak of its run if that is a character
    for (int base = 0; base < Ti; base += 64) {
        const int t = base + lane;
        const bool valid = t < Ti;
        const int c = valid ? am[t] : -2;
        int key = valid ? order_key(av[t]) : (int)0x80000000;
        int prev = __shfl_up(c, 1, 64);
        if (lane == 0) prev = carry_c;
        const bool start = valid && c != prev;
        const unsigned long long S = __ballot(start);
        const int nvalid = min(64, Ti - base);
        const bool last_round = base + 64 >= Ti;
        const bool emit = start && c != 0;
        const unsigned long long E = __ballot(emit);
        const int slot = count + __popcll(E & below);
        // inclusive max scan within segments; a segment begins at a start bit, and at lane 0 for the steps that continue the carried run
        const int head = 63 - __clzll((S | 1ULL) & (below | (1ULL << lane)));
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int other = __shfl_up(key, o, 64);
            if (lane - o >= head) key = max(key, other);
        }
        // the carried run: it goes on for `cont` steps of this round and ends here if a start bit follows or the sample does
        const int cont = S ? __builtin_ctzll(S) : nvalid;
        if (carry_slot >= 0) {
            int k = carry_key;
            if (cont > 0) k = max(k, __shfl(key, cont - 1, 64));
            if (S != 0ULL || last_round) {
                if (lane == 0) t1[out + carry_slot] = base + cont - 1, peak[out + carry_slot] = key_value(k);
            } else {
                carry_key = k;  // the whole round continues it
            }
        }
        // the runs that start in this round
        const unsigned long long after = S & ~(below | (1ULL << lane));  // start bits behind this lane
        const int end = after ? __builtin_ctzll(after) - 1 : nvalid - 1;
        const int seg = __shfl(key, end, 64);  // the scan's value at the run's last lane of this round: the maximum from its start to there
        if (emit) {
            labels[out + slot] = c;
            t0[out + slot] = t;
            if (after != 0ULL || last_round) t1[out + slot] = base + end, peak[out + slot] = key_value(seg);
        }
        if (S != 0ULL) {  // the last run that started here is the one the next round may continue
            const int ls = 63 - __clzll(S);
            const int lc = __shfl(c, ls, 64);
            carry_slot = lc != 0 ? __shfl(slot, ls, 64) : -1;
            carry_key = __shfl(seg, ls, 64);
        }
        carry_c = __shfl(c, nvalid - 1, 64);
        count += __popcll(E);
    }
    if (lane == 0) lens[row0 + n] = count;
}

// ---- character boxes: rule (b) ---------------------------------------------------------------------------------------------------------
// One workgroup per row p of the span arrays; the row is the crop of quad i = plan[p][7], whose frame is workgroup-uniform.  One lane = one
// character: two 16-byte stores for its quad.
__global__ __launch_bounds__(64) void k_char_boxes(const float* __restrict__ quads, const int* __restrict__ plan, long cap, int ld, const int* __restrict__ lens,
                                                   const int* __restrict__ t0, const int* __restrict__ t1, float* __restrict__ s0, float* __restrict__ s1,
                                                   float* __restrict__ cquads) {
    const long p = blockIdx.x;
    const long i = plan[p * 8 + 7];
    if (i < 0 || i >= cap) return;
    const int len = min(max(lens[p], 0), ld);
    if (len == 0) return;
    const CropFrame f = crop_frame(quads + i * 8);
    const int ow = max(plan[i * 8 + 2], 1);
    const float vx = -f.uy, vy = f.ux;
    for (int k = threadIdx.x; k < len; k += 64) {
        const long e = p * ld + k;
        const int a0 = min(max(4 * t0[e] - 2, 0), ow), a1 = min(max(4 * t1[e] + 2, 0), ow);
        const float c0 = (float)a0 / (float)ow * f.lng, c1 = (float)a1 / (float)ow * f.lng;
        s0[e] = c0, s1[e] = c1;
        const float r = f.sht;
        float4* q = reinterpret_cast<float4*>(cquads) + 2 * e;
        q[0] = make_float4(f.ox + c0 * f.ux, f.oy + c0 * f.uy, f.ox + c1 * f.ux, f.oy + c1 * f.uy);  // (r = 0: the terms in v vanish)
        q[1] = make_float4(f.ox + c1 * f.ux + r * vx, f.oy + c1 * f.uy + r * vy, f.ox + c0 * f.ux + r * vx, f.oy + c0 * f.uy + r * vy);
    }
}

// ---- words: rule (c) -------------------------------------------------------------------------------------------------------------------
// lo / hi of a word's four corners along the line's axis
__device__ __forceinline__ void word_extent(const float* __restrict__ q, const CropFrame& f, float& lo, float& hi) {
    const float4 a = reinterpret_cast<const float4*>(q)[0], c = reinterpret_cast<const float4*>(q)[1];
    const float p0 = (a.x - f.ox) * f.ux + (a.y - f.oy) * f.uy, p1 = (a.z - f.ox) * f.ux + (a.w - f.oy) * f.uy;
    const float p2 = (c.x - f.ox) * f.ux + (c.y - f.oy) * f.uy, p3 = (c.z - f.ox) * f.ux + (c.w - f.oy) * f.uy;
    lo = fminf(fminf(p0, p1), fminf(p2, p3));
    hi = fmaxf(fmaxf(p0, p1), fmaxf(p2, p3));
}
// (chars_below() and store_word_range() are char_range.h's: k_word_chars_chain of line_chain.hip ends the same way)
// One wave per line l (four lines per workgroup), lane j of round r holds word 64 r + j of the line's chain.  B_j, the running maximum of the
// boundaries b_j = 0.5f * (hi_j + lo_{j+1}), is an inclusive max scan across the lanes with the last lane's value carried into the next round.
// Word j owns the characters with B_{j-1} <= centre < B_j (no lower bound for the first word, no upper bound for the last), then gives up
// the spaces at both ends.
__global__ __launch_bounds__(256) void k_word_chars(const float* __restrict__ words, long wcap, const float* __restrict__ line_quads, const int* __restrict__ n_lines,
                                                    long cap, const int* __restrict__ line_offsets, const int* __restrict__ word_order, const int* __restrict__ plan,
                                                    long rows, int ld, const int* __restrict__ labels, const int* __restrict__ lens, const float* __restrict__ s0,
                                                    const float* __restrict__ s1, int space, int* __restrict__ word_chars) {
    const int lane = threadIdx.x & 63;
    const long l = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (l >= min((long)max(*n_lines, 0), cap)) return;  // (wave-uniform; the kernel has no barrier)
    const long p = plan[l * 8 + 6];
    if (p < 0 || p >= rows) return;
    const int off = line_offsets[l], m = line_offsets[l + 1] - off;
    if (off < 0 || m <= 0 || (long)off + m > wcap) return;
    const CropFrame f = crop_frame(line_quads + l * 8);
    const int nch = min(max(lens[p], 0), ld);
    const int* lab = labels + p * ld;
    const float* c0 = s0 + p * ld;
    const float* c1 = s1 + p * ld;
    float carry = -__builtin_huge_valf();  // B of the last word of the round before
    for (int base = 0; base < m; base += 64) {
        const int j = base + lane;
        const bool live = j < m;
        long w = -1;
        float B = -__builtin_huge_valf();
        if (live) {
            w = word_order[off + j];
            if (w < 0 || w >= wcap) w = -1;
        }
        if (live && j + 1 < m && w >= 0) {
            const long wn = word_order[off + j + 1];
            if (wn >= 0 && wn < wcap) {
                float lo, hi, lo_n, hi_n;
                word_extent(words + w * 8, f, lo, hi);
                word_extent(words + wn * 8, f, lo_n, hi_n);
                B = 0.5f * (hi + lo_n);
            }
        }
        if (lane == 0) B = fmaxf(B, carry);
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float other = __shfl_up(B, o, 64);
            if (lane >= o) B = fmaxf(B, other);
        }
        float below = __shfl_up(B, 1, 64);  // B_{j-1}
        if (lane == 0) below = carry;
        carry = __shfl(B, 63, 64);
        if (w >= 0) {
            int first = j == 0 ? 0 : chars_below(c0, c1, nch, below);
            const int end = j == m - 1 ? nch : chars_below(c0, c1, nch, B);
            store_word_range(lab, first, end, space, word_chars, w);
        }
    }
}

}  // namespace

extern "C" {

int ocrs_ctc_decode_spans(const float* lp, const long long* in_len, int* amax, float* amax_lp, int T, int N, int C, long row0, int ld, int* labels, int* t0, int* t1,
                          float* peak, int* lens, hipStream_t st) {
    OCRS_CHECK_ARG(T > 0 && N >= 0 && C > 0 && row0 >= 0 && ld >= T && (long)T * N < (1L << 31) * 16);
    if (N == 0) return OCRS_OK;
    OCRS_CHECK_ARG(lp && in_len && amax && amax_lp && labels && t0 && t1 && peak && lens);
    const long rows = (long)T * N;
    hipLaunchKernelGGL(k_argmax_peak, dim3((unsigned)((rows + 15) / 16)), dim3(256), 0, st, lp, amax, amax_lp, T, N, C);
    hipLaunchKernelGGL(k_ctc_spans, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, (const int*)amax, (const float*)amax_lp, in_len, T, N, row0, ld, labels, t0, t1,
                       peak, lens);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

int ocrs_char_boxes(const float* quads, const int* plan, long cap, long rows, int ld, const int* lens, const int* t0, const int* t1, float* s0, float* s1,
                    float* char_quads, hipStream_t st) {
    OCRS_CHECK_ARG(cap >= 0 && rows >= 0 && rows <= cap && rows < (1L << 31) && ld > 0);
    if (rows == 0) return OCRS_OK;
    OCRS_CHECK_ARG(quads && plan && lens && t0 && t1 && s0 && s1 && char_quads && aligned16(quads) && aligned16(char_quads));
    hipLaunchKernelGGL(k_char_boxes, dim3((unsigned)rows), dim3(64), 0, st, quads, plan, cap, ld, lens, t0, t1, s0, s1, char_quads);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

int ocrs_word_chars(const float* words, long wcap, const float* line_quads, const int* n_lines, long cap, const int* line_offsets, const int* word_order,
                    const int* plan, long rows, int ld, const int* labels, const int* lens, const float* s0, const float* s1, int space, int* word_chars,
                    hipStream_t st) {
    OCRS_CHECK_ARG(wcap >= 0 && cap >= 0 && cap <= wcap && rows >= 0 && rows <= cap && cap < (1L << 31) && ld > 0);
    if (cap == 0 || rows == 0) return OCRS_OK;
    OCRS_CHECK_ARG(words && line_quads && n_lines && line_offsets && word_order && plan && labels && lens && s0 && s1 && word_chars);
    OCRS_CHECK_ARG(aligned16(words) && aligned16(line_quads) && (reinterpret_cast<uintptr_t>(word_chars) & 7) == 0);
    hipLaunchKernelGGL(k_word_chars, dim3((unsigned)((cap + 3) / 4)), dim3(256), 0, st, words, wcap, line_quads, n_lines, cap, line_offsets, word_order, plan, rows, ld,
                       labels, lens, s0, s1, space, word_chars);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

}  // extern "C"
