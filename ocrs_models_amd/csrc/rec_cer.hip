// Character error rate of the recognition loops on the device (gfx950): batched Levenshtein distance and the fused
// RecognitionAccuracyStats.update (ocrs_models/train_rec.py:29-68 with decode_text / ctc_greedy_decode_text, datasets/util.py:132-177):
// arg-max -> CTC collapse -> target compaction -> edit distance -> two int64 counters.  Integers only: every result is exact.
//
// Edit distance: ONE WAVE PER SAMPLE, anti-diagonal sweep.  Sequence b lies along the lanes, 64 columns per pass (lane j owns column
// c0 + j); sequence a is streamed through the rows.  At diagonal step d lane j computes D[d - j + 1][c0 + j + 1] from
//   up   = its own value of the previous step,
//   left = lane j-1's value of the previous step  (ONE DPP wave shift),
//   diag = the `left` it received one step earlier,
// and a's label for that row arrives through a second DPP shift of the label register (lane 0 injects a[d]).  Lane 0's left neighbour is
// the boundary column D[.][c0]: the row index in pass 0, and what lane 63 of the previous pass stored to the workspace otherwise.  Labels
// and boundary values reach lane 0 through v_readlane from a 64-entry register chunk that all lanes load together (the next chunk is
// prefetched one chunk ahead), so no step waits for memory.  A pass is m + 63 steps of ~12 VALU instructions; longer b = more passes, longer
// a = more steps: no LDS, a fixed handful of registers, no limit on either length and no second code path.
#include "common.h"
#include "edit_distance.h"  // wave_shr1, code_of, wave_edit_distance (shared with ocr_eval.hip)

namespace {

__device__ __forceinline__ int clamp_len(long long v, int hi) { return v < 0 ? 0 : (v > hi ? hi : (int)v); }

__global__ __launch_bounds__(64) void k_edit_distance(const int* a, const long long* __restrict__ a_len, int pa, const int* b,
                                                      const long long* __restrict__ b_len, int pb, const int* __restrict__ codes, int ncodes,
                                                      int* ws, int* __restrict__ dist) {
    const int n = blockIdx.x, lane = threadIdx.x;
    const int m = __builtin_amdgcn_readfirstlane(clamp_len(a_len[n], pa)), nb = __builtin_amdgcn_readfirstlane(clamp_len(b_len[n], pb));
    const int d = wave_edit_distance(a + (long)n * pa, m, b + (long)n * pb, nb, codes, ncodes, ws + (long)n * pa, lane);
    if (lane == 0) dist[n] = d;
}

// arg-max over the classes, first maximum on ties (the comparison of rec_seq.hip's k_argmax): amax [N][T]
__global__ __launch_bounds__(256) void k_cer_argmax(const float* __restrict__ lp, int* __restrict__ amax, int T, int N, int C) {
    const int sub = threadIdx.x & 15;
    const long row = (long)blockIdx.x * 16 + (threadIdx.x >> 4);  // row = t*N + n
    if (row >= (long)T * N) return;
    float best = -INFINITY;
    int bi = C;
    for (int c = sub; c < C; c += 16) {
        const float v = lp[row * C + c];
        if (v > best || (v == best && c < bi)) best = v, bi = c;
    }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ov > best || (ov == best && oi < bi)) best = ov, bi = oi;
    }
    if (sub == 0) {
        const int t = (int)(row / N), n = (int)(row - (long)t * N);
        amax[(long)n * T + t] = bi;
    }
}

// left-aligned copy of the kept entries of one 64-wide chunk (ballot prefix): returns the new count
__device__ __forceinline__ int wave_compact(int* out, int cnt, int v, bool keep, int lane) {
    const unsigned long long mask = __ballot(keep);
    if (keep) out[cnt + __popcll(mask & ((1ull << lane) - 1ull))] = v;
    return cnt + __popcll(mask);
}

// One wave per sample: collapse (repeat test before the blank test, in_len clamped to [0, T]), target compaction (decode_text: every entry
// <= 0 of the WHOLE padded row is dropped, tgt_len plays no part), edit distance, counters.
__global__ __launch_bounds__(64) void k_cer_update(const int* __restrict__ amax, const long long* __restrict__ in_len, const int* __restrict__ targets,
                                                   const long long* __restrict__ tgt_len, const int* __restrict__ codes, int* labels, int* tcomp,
                                                   int* bnd, unsigned long long* state, int* __restrict__ dist, int T, int C, int Lpitch) {
    const int n = blockIdx.x, lane = threadIdx.x;
    const int Ti = __builtin_amdgcn_readfirstlane(clamp_len(in_len[n], T));
    int* lab = labels + (long)n * T;
    int* tc = tcomp + (long)n * Lpitch;
    int m = 0, prev_last = -1;
    for (int t0 = 0; t0 < Ti; t0 += 64) {
        const int t = t0 + lane;
        const int c = t < Ti ? amax[(long)n * T + t] : 0;
        const int prev = wave_shr1(prev_last, c);
        m = wave_compact(lab, m, c, t < Ti && c != prev && c != 0, lane);
        prev_last = __builtin_amdgcn_readlane(c, 63);
    }
    int nt = 0;
    for (int l0 = 0; l0 < Lpitch; l0 += 64) {
        const int l = l0 + lane;
        const int x = l < Lpitch ? targets[(long)n * Lpitch + l] : 0;
        nt = wave_compact(tc, nt, x, x > 0, lane);
    }
    __syncthreads();  // (one-wave block) the compacted rows are read back by other lanes
    const int d = wave_edit_distance(lab, __builtin_amdgcn_readfirstlane(m), tc, __builtin_amdgcn_readfirstlane(nt), codes, C, bnd + (long)n * T, lane);
    if (lane == 0) {
        atomicAdd(&state[0], (unsigned long long)d);
        atomicAdd(&state[1], (unsigned long long)tgt_len[n]);  // the lengths as given (the reference's sum(target_lengths))
        if (dist) dist[n] = d;
    }
}

}  // namespace

extern "C" {

// Levenshtein distance per row pair (RecognitionAccuracyStats.update's levenshtein(), train_rec.py:29-68).
long ocrs_edit_distance_ws_bytes(int N, int pa) { return N < 1 || pa < 0 ? 0 : (long)N * (pa > 0 ? pa : 1) * 4; }

int ocrs_edit_distance(const int* a, const long long* a_len, int pa, const int* b, const long long* b_len, int pb, const int* codes, int ncodes,
                       void* ws, int* dist, int N, hipStream_t st) {
    OCRS_CHECK_ARG(a_len && b_len && ws && dist && N > 0 && pa >= 0 && pb >= 0 && (a || pa == 0) && (b || pb == 0));
    OCRS_CHECK_ARG(codes ? ncodes > 0 : ncodes == 0);
    hipLaunchKernelGGL(k_edit_distance, dim3(N), dim3(64), 0, st, a, a_len, pa, b, b_len, pb, codes, ncodes, (int*)ws, dist);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

// workspace of ocrs_ctc_cer_update: arg-max [N][T] | collapsed labels [N][T] | boundary column [N][T] | compacted targets [N][Lpitch], int32
long ocrs_ctc_cer_ws_bytes(int T, int N, int Lpitch) { return T < 1 || N < 1 || Lpitch < 0 ? 0 : (long)N * (3L * T + Lpitch) * 4; }

int ocrs_ctc_cer_update(const float* lp, const long long* in_len, const int* targets, const long long* tgt_len, const int* codes, void* ws,
                        long long* state, int* dist, int T, int N, int C, int Lpitch, hipStream_t st) {
    OCRS_CHECK_ARG(lp && in_len && tgt_len && ws && state && T > 0 && N > 0 && C > 0 && Lpitch >= 0 && (targets || Lpitch == 0));
    int* amax = static_cast<int*>(ws);
    int* labels = amax + (long)N * T;
    int* bnd = labels + (long)N * T;
    int* tcomp = bnd + (long)N * T;
    const long rows = (long)T * N;
    OCRS_CHECK_ARG((rows + 15) / 16 < (1L << 31));
    hipLaunchKernelGGL(k_cer_argmax, dim3((unsigned)((rows + 15) / 16)), dim3(256), 0, st, lp, amax, T, N, C);
    hipLaunchKernelGGL(k_cer_update, dim3(N), dim3(64), 0, st, amax, in_len, targets, tgt_len, codes, labels, tcomp, bnd,
                       reinterpret_cast<unsigned long long*>(state), dist, T, C, Lpitch);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

}  // extern "C"
