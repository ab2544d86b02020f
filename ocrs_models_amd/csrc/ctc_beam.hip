// CTC prefix beam search and forced alignment (Python: text.beam_decode_spans / ctc_align_spans; restated for the tests in
// tests/beam_ref.py): the most probable labelling of a crop instead of the labelling of its most probable alignment, with the span arrays of
// char_spans.hip filled for it.
//
//   k_ctc_beam    one workgroup per sample, the beam (at most 64 prefixes) in LDS, the prefix tree in the workspace.  Thread = (label c,
//                 slot group g): candidate (slot i, label c) is a function of the slot's three numbers and lp[t][c], which the thread keeps in
//                 a register, so the W * C candidates are recomputed by every pass and never stored.  The W best by (total descending,
//                 candidate index ascending) come from a radix select over the 48-bit composite (order key of the total | 65535 - index):
//                 one LDS histogram of 256 bins per 8-bit digit, at most six passes, ending at the first digit whose bin is taken whole
//                 (the usual case after one or two).  The survivors are ranked inside one wave by counting larger composites.
//                 k_ctc_beam<true> (Python: lm= of text.beam_decode_spans; restated in tests/beam_lm_ref.py) ranks by
//                 total + the gains of a character n-gram table instead of the total alone; k_ctc_beam<false> is the kernel of §18.
//   k_ctc_align   one wave per sample, lanes over the 2 L + 1 states of blank | l1 | blank | ... | lL | blank, T sequential steps with the two
//                 delta rows in LDS; the 2-bit back-pointers of a step leave as two ballots per 64 states.  Lane 0 walks them back.
//
// Integer LDS atomics only (histogram counts and the survivors' list positions, neither of which reaches a result): equal input gives
// equal bytes.  Every loop is bounded by T, W, C or L; nothing waits for another workgroup.
#include "common.h"

namespace {

constexpr float NEG_INF = -__builtin_huge_valf();
constexpr int BEAM_MAX_W = 64, BEAM_MAX_C = 256, BEAM_THREADS = 256;
constexpr int ALIGN_MAX_R = 100;  // rounds of 64 states whose LDS (10 bytes per state) stays below 64 KiB

// fp32 -> unsigned with the same order (-0 first folded into +0)
__device__ __forceinline__ unsigned ukey(float v) {
    const int b = __float_as_int(v + 0.0f);
    return (unsigned)(b ^ ((b >> 31) & 0x7fffffff)) ^ 0x80000000u;
}
__device__ __forceinline__ int order_key(float v) {
    const int b = __float_as_int(v);
    return b ^ ((b >> 31) & 0x7fffffff);
}
__device__ __forceinline__ float key_value(int k) { return __int_as_float(k ^ ((k >> 31) & 0x7fffffff)); }

// log(exp(a) + exp(b)) with the hardware exp2 / log2; (-inf, -inf) -> -inf
__device__ __forceinline__ float logaddexp(float a, float b) {
    const float m = fmaxf(a, b), n = fminf(a, b);
    if (m == NEG_INF) return NEG_INF;
    return m + 0.6931471805599453f * __builtin_amdgcn_logf(1.0f + __builtin_amdgcn_exp2f((n - m) * 1.4426950408889634f));
}

// ---- prefix beam search ------------------------------------------------------------------------------------------------------------------
// nodes [N][T * W + 1] (parent node, label): node 0 is the empty prefix, node 1 + t W + r the prefix that step t created at rank r.
//
// LM = true: every slot also carries lm, the fp32 sum of the gains of its labels, last2, the label before its last, and the
// offset of its context's row in the gain table; a candidate's rank is its total + lm (+ gain[row + c] for an extension), read again by every
// pass like lp[t][c] is recomputed.  LM = false is the kernel of §18: none of the additions below is instantiated.
template <bool LM>
__global__ __launch_bounds__(BEAM_THREADS) void k_ctc_beam(const float* __restrict__ lp, const long long* __restrict__ in_len, int T, int N, int C, int W, int cshift,
                                                           long row0, int ld, int* __restrict__ labels, int* __restrict__ lens, float* __restrict__ score,
                                                           int2* __restrict__ nodes_all, const float* __restrict__ gain, int order,
                                                           float* __restrict__ lm_score) {
    __shared__ float s_lm[LM ? 2 : 1][LM ? BEAM_MAX_W : 1];
    __shared__ int s_l2[LM ? 2 : 1][LM ? BEAM_MAX_W : 1];
    __shared__ float2 s_lmrow[LM ? BEAM_MAX_W : 1];  // lm | offset of the context's row in gain (bits)
    __shared__ float s_lb[2][BEAM_MAX_W], s_lnb[2][BEAM_MAX_W];
    __shared__ int s_node[2][BEAM_MAX_W], s_par[2][BEAM_MAX_W], s_last[2][BEAM_MAX_W];
    __shared__ float4 s_slot[BEAM_MAX_W];  // lb | total | last label (bits) | total of the stay candidate
    __shared__ float s_tot[BEAM_MAX_W], s_stlb[BEAM_MAX_W], s_stlnb[BEAM_MAX_W], s_lp[BEAM_MAX_C];
    __shared__ int s_qs[BEAM_MAX_W];
    __shared__ __attribute__((aligned(16))) unsigned s_hist[256];
    __shared__ unsigned long long s_scomp[BEAM_MAX_W];
    __shared__ unsigned s_cnt;
    __shared__ int s_sel[4], s_nb;

    const int tid = threadIdx.x, n = blockIdx.x;
    const long long il = in_len[n];
    const int Ti = il < 0 ? 0 : (il > T ? T : (int)il);
    int2* nodes = nodes_all + (long)n * ((long)T * W + 1);
    const int c = tid & ((1 << cshift) - 1), g = tid >> cshift, G = BEAM_THREADS >> cshift;
    const bool live = c < C;
    if (tid == 0) {
        s_lb[0][0] = 0.f, s_lnb[0][0] = NEG_INF, s_node[0][0] = 0, s_par[0][0] = -1, s_last[0][0] = 0;
        s_nb = 1;
        nodes[0] = make_int2(-1, 0);
        if constexpr (LM) s_lm[0][0] = 0.f, s_l2[0][0] = 0;
    }
    float lpn = (live && Ti > 0) ? lp[(long)n * C + c] : NEG_INF;
    __syncthreads();
    int cur = 0;
    for (int t = 0; t < Ti; ++t) {
        const float lpc = lpn;
        if (live && t + 1 < Ti) lpn = lp[((long)(t + 1) * N + n) * C + c];
        const int nb = s_nb;
        // totals, and for every prefix the slot of its parent (the prefix without its last label), if that is in the beam
        if (g == 0 && live) s_lp[c] = lpc;
        if (tid < nb) {
            s_tot[tid] = logaddexp(s_lb[cur][tid], s_lnb[cur][tid]);
            const int par = s_par[cur][tid];
            int q = -1;
            for (int i = 0; i < nb; ++i)
                if (s_node[cur][i] == par) q = i;
            s_qs[tid] = q;
        }
        if (tid == 0) s_cnt = 0;
        __syncthreads();
        // the stay candidates with their merges; per thread, the slots whose extension by c is another slot's prefix
        if (tid < nb) {
            const int e = s_last[cur][tid], q = s_qs[tid];
            const float lb = s_lb[cur][tid], tot = s_tot[tid];
            const float stlb = tot + s_lp[0];
            float stlnb = e == 0 ? NEG_INF : s_lnb[cur][tid] + s_lp[e];
            if (q >= 0) stlnb = logaddexp(stlnb, (s_last[cur][q] == e ? s_lb[cur][q] : s_tot[q]) + s_lp[e]);
            s_stlb[tid] = stlb, s_stlnb[tid] = stlnb;
            s_slot[tid] = make_float4(lb, tot, __int_as_float(e), logaddexp(stlb, stlnb));
            if constexpr (LM) {
                const int ro = order == 3 ? (s_l2[cur][tid] * C + e) * C : (order == 2 ? e * C : 0);
                s_lmrow[tid] = make_float2(s_lm[cur][tid], __int_as_float(ro));
            }
        }
        unsigned long long sup = 0ULL;
        if (live && c != 0)
            for (int j = 0; j < nb; ++j)
                if (s_last[cur][j] == c && s_qs[j] >= 0) sup |= 1ULL << s_qs[j];
        s_hist[tid] = 0u;
        __syncthreads();
        // candidate (i, c): index i C + c; c = 0 is the stay.  -> exists, composite = order key of its total (LM: its rank) | 65535 - index
        auto cand = [&](int i, unsigned long long& comp) -> bool {
            const float4 s = s_slot[i];
            float v;
            if (c == 0) {
                v = s.w;
            } else {
                if ((sup >> i) & 1ULL) return false;
                v = (__float_as_int(s.z) == c ? s.x : s.y) + lpc;
            }
            if (!(v > NEG_INF)) return false;
            if constexpr (LM) {  // rank = total + lm'; an extension's lm' = lm + gain[row + c], the add the new slot repeats
                const float2 m = s_lmrow[i];
                v += c == 0 ? m.x : m.x + gain[__float_as_int(m.y) + c];
                if (!(v > NEG_INF)) return false;
            }
            comp = ((unsigned long long)ukey(v) << 16) | (unsigned long long)(0xFFFF - (i * C + c));
            return true;
        };
        // radix select of the K-th largest composite, K = min(W, candidates)
        unsigned long long prefix = 0ULL;
        int sh = 40, K = 0;
        for (int pass = 0; pass < 6; ++pass) {
            if (pass > 0) {
                s_hist[tid] = 0u;
                __syncthreads();
            }
            if (live)
                for (int i = g; i < nb; i += G) {
                    unsigned long long comp;
                    if (cand(i, comp) && (pass == 0 || (comp >> (sh + 8)) == prefix)) atomicAdd(&s_hist[(unsigned)(comp >> sh) & 255u], 1u);
                }
            __syncthreads();
            if (tid < 64) {  // wave 0: lane l holds bins 4 l .. 4 l + 3; suffix sums from the top bin down
                const uint4 h = reinterpret_cast<const uint4*>(s_hist)[tid];
                const unsigned own = h.x + h.y + h.z + h.w;
                unsigned incl = own;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const unsigned other = __shfl_down(incl, o, 64);
                    if (tid + o < 64) incl += other;
                }
                const unsigned all = __shfl(incl, 0, 64);
                const unsigned want = pass == 0 ? min((unsigned)W, all) : (unsigned)s_sel[1];
                unsigned above = incl - own;
                if (want > 0u && above < want && want <= incl) {  // the one lane whose bins hold the want-th largest
                    int b = 3;
                    unsigned hb = h.w;
                    if (above + hb < want) above += hb, b = 2, hb = h.z;
                    if (above + hb < want) above += hb, b = 1, hb = h.y;
                    if (above + hb < want) above += hb, b = 0, hb = h.x;
                    s_sel[0] = 4 * tid + b, s_sel[1] = (int)(want - above), s_sel[2] = (int)hb;
                }
                if (tid == 0 && want == 0u) s_sel[0] = 0, s_sel[1] = 0, s_sel[2] = 0;
                if (tid == 0 && pass == 0) s_sel[3] = (int)want;
            }
            __syncthreads();
            if (pass == 0) K = s_sel[3];
            prefix = (prefix << 8) | (unsigned long long)s_sel[0];
            if (s_sel[2] == s_sel[1] || sh == 0) break;  // the bin is taken whole: everything from its lowest composite up survives
            sh -= 8;
        }
        const unsigned long long thr = prefix << sh;
        if (live && K > 0)
            for (int i = g; i < nb; i += G) {
                unsigned long long comp;
                if (cand(i, comp) && comp >= thr) {
                    const unsigned pos = atomicAdd(&s_cnt, 1u);
                    if (pos < (unsigned)BEAM_MAX_W) s_scomp[pos] = comp;
                }
            }
        __syncthreads();
        // wave 0: rank = number of larger composites (they are distinct); the new beam goes into the other buffer
        if (tid < 64) {
            const int nxt = cur ^ 1;
            const unsigned long long my = tid < K ? s_scomp[tid] : 0ULL;
            int rank = 0;
            for (int j = 0; j < K; ++j) rank += __shfl(my, j, 64) > my ? 1 : 0;
            if (tid < K) {
                const int idx = 0xFFFF - (int)(my & 0xFFFFULL);
                const int i = idx / C, cc = idx - i * C;
                if (cc == 0) {
                    s_lb[nxt][rank] = s_stlb[i], s_lnb[nxt][rank] = s_stlnb[i];
                    s_node[nxt][rank] = s_node[cur][i], s_par[nxt][rank] = s_par[cur][i], s_last[nxt][rank] = s_last[cur][i];
                    if constexpr (LM) s_lm[nxt][rank] = s_lm[cur][i], s_l2[nxt][rank] = s_l2[cur][i];
                } else {
                    const float4 s = s_slot[i];
                    const int node = 1 + t * W + rank;
                    s_lb[nxt][rank] = NEG_INF, s_lnb[nxt][rank] = ((__float_as_int(s.z) == cc ? s.x : s.y) + s_lp[cc]) + 0.0f;
                    s_node[nxt][rank] = node, s_par[nxt][rank] = s_node[cur][i], s_last[nxt][rank] = cc;
                    nodes[node] = make_int2(s_node[cur][i], cc);
                    if constexpr (LM) {
                        const float2 m = s_lmrow[i];
                        s_lm[nxt][rank] = m.x + gain[__float_as_int(m.y) + cc], s_l2[nxt][rank] = s_last[cur][i];
                    }
                }
            }
            if (tid == 0) s_nb = K;
        }
        __syncthreads();
        cur ^= 1;
    }
    if (tid == 0) {
        const long out = (row0 + n) * (long)ld;
        if (s_nb == 0) {  // every candidate of some step was at -inf
            lens[row0 + n] = 0, score[row0 + n] = NEG_INF;
            if constexpr (LM) lm_score[row0 + n] = 0.f;
        } else {
            int len = 0;
            for (int x = s_node[cur][0]; x > 0 && len < Ti; x = nodes[x].x) ++len;
            int x = s_node[cur][0];
            for (int k = len - 1; k >= 0; --k) {
                const int2 nd = nodes[x];
                labels[out + k] = nd.y;
                x = nd.x;
            }
            lens[row0 + n] = len;
            score[row0 + n] = logaddexp(s_lb[cur][0], s_lnb[cur][0]);
            if constexpr (LM) lm_score[row0 + n] = s_lm[cur][0];
        }
    }
}

// ---- forced alignment --------------------------------------------------------------------------------------------------------------------
// bp [N][T][Rcap][2] 64-bit words: bit s & 63 of word 0 / 1 of round s >> 6 = low / high bit of state s' step back (0 stay, 1, 2).
__global__ __launch_bounds__(64) void k_ctc_align(const float* __restrict__ lp, const long long* __restrict__ in_len, int T, int N, int C, long row0, int ld,
                                                  const int* __restrict__ labels, int* __restrict__ lens, int* __restrict__ t0, int* __restrict__ t1,
                                                  float* __restrict__ peak, unsigned long long* __restrict__ bp_all, int Rcap) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x, n = blockIdx.x;
    const int Scap = Rcap * 64;
    float* dprev = smem;
    float* dcur = smem + Scap;
    int* s_lab = reinterpret_cast<int*>(smem + 2 * Scap);  // Scap / 2 labels
    const long long il = in_len[n];
    const int Ti = il < 0 ? 0 : (il > T ? T : (int)il);
    const int L = lens[row0 + n];
    if (L < 0 || (L == 0 && Ti == 0)) return;  // (uniform) nothing to align
    const long out = (row0 + n) * (long)ld;
    if (L > Ti || 2 * L + 1 > Scap) {  // (uniform) fewer steps than labels, or more labels than the workspace was sized for
        if (lane == 0) lens[row0 + n] = -1;
        return;
    }
    bool bad = false;
    for (int k = lane; k < L; k += 64) {
        const int v = labels[out + k];
        s_lab[k] = v;
        bad |= v < 1 || v >= C;
    }
    if (__any(bad)) {
        if (lane == 0) lens[row0 + n] = -1;
        return;
    }
    __syncthreads();
    const int S = 2 * L + 1, R = (S + 63) >> 6;
    unsigned long long* bp = bp_all + (long)n * T * Rcap * 2;
    {
        const float* row = lp + (long)n * C;
        for (int s = lane; s < S; s += 64) dprev[s] = s == 0 ? row[0] : (s == 1 ? row[s_lab[0]] : NEG_INF);
    }
    __syncthreads();
    for (int t = 1; t < Ti; ++t) {
        const float* row = lp + ((long)t * N + n) * C;
        for (int r = 0; r < R; ++r) {
            const int s = lane + 64 * r;
            int b = 0;
            if (s < S) {
                const int e = (s & 1) ? s_lab[s >> 1] : 0;
                float v = dprev[s];
                if (s >= 1 && dprev[s - 1] > v) v = dprev[s - 1], b = 1;
                if (s >= 2 && e != 0 && e != s_lab[(s >> 1) - 1] && dprev[s - 2] > v) v = dprev[s - 2], b = 2;
                dcur[s] = row[e] + v;
            }
            const unsigned long long b0 = __ballot(b & 1), b1 = __ballot(b >> 1);
            if (lane == 0) {
                unsigned long long* w = bp + ((long)t * Rcap + r) * 2;
                w[0] = b0, w[1] = b1;
            }
        }
        __syncthreads();
        float* sw = dprev;
        dprev = dcur, dcur = sw;
    }
    const float e2 = dprev[2 * L], e1 = L > 0 ? dprev[2 * L - 1] : NEG_INF;
    const int s_end = e1 > e2 ? 2 * L - 1 : 2 * L;
    if (!(fmaxf(e1, e2) > NEG_INF)) {  // (uniform) no alignment of finite score
        if (lane == 0) lens[row0 + n] = -1;
        return;
    }
    if (lane != 0) return;
    int s = s_end, kc = -1, first = 0, key = 0;
    for (int t = Ti - 1; t >= 0; --t) {
        const int k = (s & 1) ? (s >> 1) : -1;
        if (k != kc) {
            if (kc >= 0) t0[out + kc] = first, peak[out + kc] = key_value(key);
            kc = k;
            if (k >= 0) t1[out + k] = t, key = (int)0x80000000;
        }
        if (k >= 0) {
            first = t;
            key = max(key, order_key(lp[((long)t * N + n) * C + s_lab[k]]));
        }
        if (t > 0) {
            const unsigned long long* w = bp + ((long)t * Rcap + (s >> 6)) * 2;
            s -= (int)((w[0] >> (s & 63)) & 1ULL) + 2 * (int)((w[1] >> (s & 63)) & 1ULL);
        }
    }
    if (kc >= 0) t0[out + kc] = first, peak[out + kc] = key_value(key);
}

inline int align_rounds(int T, int L) { return (2 * (L < T ? L : T) + 1 + 63) / 64; }

}  // namespace

extern "C" {

long ocrs_ctc_beam_ws_bytes(int T, int N, int W) {
    return T < 1 || N < 1 || W < 1 || W > BEAM_MAX_W || (long)T * W >= (1L << 31) - 1 ? 0 : (long)N * ((long)T * W + 1) * 8;
}

long ocrs_ctc_align_ws_bytes(int T, int N, int Lmax) { return T < 1 || N < 1 || Lmax < 0 ? 0 : (long)N * T * align_rounds(T, Lmax) * 16; }

int ocrs_ctc_beam_decode(const float* lp, const long long* in_len, int T, int N, int C, int W, long row0, int ld, int* labels, int* lens, float* score, void* ws,
                         long ws_bytes, hipStream_t st) {
    OCRS_CHECK_ARG(W >= 1 && W <= BEAM_MAX_W && C >= 2 && C <= BEAM_MAX_C);
    OCRS_CHECK_ARG(T > 0 && N >= 0 && row0 >= 0 && ld >= T && (long)T * W < (1L << 31) - 1);
    if (N == 0) return OCRS_OK;
    OCRS_CHECK_ARG(lp && in_len && labels && lens && score && ws && (reinterpret_cast<uintptr_t>(ws) & 7) == 0 && ws_bytes >= ocrs_ctc_beam_ws_bytes(T, N, W));
    int cshift = 1;
    while ((1 << cshift) < C) ++cshift;
    hipLaunchKernelGGL(k_ctc_beam<false>, dim3((unsigned)N), dim3(BEAM_THREADS), 0, st, lp, in_len, T, N, C, W, cshift, row0, ld, labels, lens, score,
                       reinterpret_cast<int2*>(ws), nullptr, 0, nullptr);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

int ocrs_ctc_beam_decode_lm(const float* lp, const long long* in_len, int T, int N, int C, int W, const float* gain, int order, long row0, int ld, int* labels,
                            int* lens, float* score, float* lm_score, void* ws, long ws_bytes, hipStream_t st) {
    OCRS_CHECK_ARG(W >= 1 && W <= BEAM_MAX_W && C >= 2 && C <= BEAM_MAX_C && order >= 1 && order <= 3);
    OCRS_CHECK_ARG(T > 0 && N >= 0 && row0 >= 0 && ld >= T && (long)T * W < (1L << 31) - 1);
    OCRS_CHECK_ARG(gain && lm_score);
    if (N == 0) return OCRS_OK;
    OCRS_CHECK_ARG(lp && in_len && labels && lens && score && ws && (reinterpret_cast<uintptr_t>(ws) & 7) == 0 && ws_bytes >= ocrs_ctc_beam_ws_bytes(T, N, W));
    int cshift = 1;
    while ((1 << cshift) < C) ++cshift;
    hipLaunchKernelGGL(k_ctc_beam<true>, dim3((unsigned)N), dim3(BEAM_THREADS), 0, st, lp, in_len, T, N, C, W, cshift, row0, ld, labels, lens, score,
                       reinterpret_cast<int2*>(ws), gain, order, lm_score);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

int ocrs_ctc_align_spans(const float* lp, const long long* in_len, int T, int N, int C, long row0, int ld, const int* labels, int* lens, int* t0, int* t1, float* peak,
                         void* ws, long ws_bytes, hipStream_t st) {
    OCRS_CHECK_ARG(T > 0 && N >= 0 && C >= 1 && row0 >= 0 && ld >= T);
    if (N == 0) return OCRS_OK;
    OCRS_CHECK_ARG(lp && in_len && labels && lens && t0 && t1 && peak && ws && (reinterpret_cast<uintptr_t>(ws) & 7) == 0 && ws_bytes > 0);
    long rcap = ws_bytes / N / (16L * T);
    if (rcap > align_rounds(T, T)) rcap = align_rounds(T, T);
    if (rcap > ALIGN_MAX_R) rcap = ALIGN_MAX_R;
    OCRS_CHECK_ARG(rcap >= 1);
    hipLaunchKernelGGL(k_ctc_align, dim3((unsigned)N), dim3(64), (size_t)rcap * 64 * 10, st, lp, in_len, T, N, C, row0, ld, labels, lens, t0, t1, peak,
                       reinterpret_cast<unsigned long long*>(ws), (int)rcap);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

}  // extern "C"
