// End-to-end accuracy of page OCR against annotated words on the device (Python: ocrs_models_amd/inference/evaluate.py; restated
// for the tests in tests/eval_ref.py): which predicted word is which annotated word, whether its text is right, and running integer sums.
//
//   pair IoU    k_ev_pairs   one thread per (prediction, annotation) pair of a page: strict bbox prefilter, zero-area exits, quad_inter and
//                            iou = inter / (pa + ga - inter) in fp64 -- the operations and order of postprocess.box_match_metrics -- into the
//                            page's dense (predictions x annotations) matrix; a prediction more than half inside an ignored annotation is flagged
//   assignment  k_ev_match   one workgroup per page: the greedy one-to-one matching under the strict total order (IoU descending, prediction
//                            ascending, annotation ascending), computed in rounds of mutually-best pairs; then the ignore rule
//   text        k_ev_text    one wave per prediction: Levenshtein distance (the wave routine of rec_cer.hip), exact and ASCII-case-folded equality
//                            of a matched pair; the prediction side of the counters
//               k_ev_truth   the annotation side of the counters
//
// All inputs are pooled over the pages of a call with offset arrays.  Nothing synchronises, nothing is allocated, every size comes from the
// host.  The matrix of a page is dense, so no candidate can be dropped and there is no capacity to overflow.  Every accumulated quantity is an
// integer: equal input gives equal bytes.  The geometry repeats the host's arithmetic, so FMA contraction is off (quad_geom.h).
#include "common.h"
#include "edit_distance.h"
#include "quad_geom.h"

#pragma clang fp contract(off)

namespace {

// the slice of one page in the pooled arrays; ok = the offsets describe rows inside the arrays and a matrix inside the pair buffer
struct EvPage {
    long p0, np, g0, ng, m0;
    bool ok;
};

__device__ __forceinline__ EvPage ev_page(const int* __restrict__ pred_offs, const int* __restrict__ gt_offs, const long long* __restrict__ pair_offs,
                                          int b, long P, long G, long n_pairs) {
    EvPage e;
    e.p0 = pred_offs[b], e.np = (long)pred_offs[b + 1] - e.p0;
    e.g0 = gt_offs[b], e.ng = (long)gt_offs[b + 1] - e.g0;
    e.m0 = pair_offs[b];
    e.ok = e.p0 >= 0 && e.np >= 0 && e.p0 + e.np <= P && e.g0 >= 0 && e.ng >= 0 && e.g0 + e.ng <= G && e.m0 >= 0 && e.m0 + e.np * e.ng <= n_pairs;
    return e;
}

__global__ __launch_bounds__(256) void k_ev_pairs(const float* __restrict__ pq, const int* __restrict__ pred_offs, const float* __restrict__ gq,
                                                  const int* __restrict__ gt_offs, const unsigned char* __restrict__ gt_ignore,
                                                  const long long* __restrict__ pair_offs, long P, long G, long n_pairs, double* __restrict__ iou,
                                                  int* __restrict__ ign_hit) {
    const EvPage e = ev_page(pred_offs, gt_offs, pair_offs, blockIdx.y, P, G, n_pairs);
    if (!e.ok) return;
    const long n = e.np * e.ng;
    for (long k = (long)blockIdx.x * 256 + threadIdx.x; k < n; k += (long)gridDim.x * 256) {
        const long i = k / e.ng, j = k - i * e.ng;
        double ax[4], ay[4], bx[4], by[4];
        load_quad(pq + (e.p0 + i) * 8, ax, ay);
        load_quad(gq + (e.g0 + j) * 8, bx, by);
        double pminx = ax[0], pmaxx = ax[0], pminy = ay[0], pmaxy = ay[0];
        for (int c = 1; c < 4; ++c) pminx = fmin(pminx, ax[c]), pmaxx = fmax(pmaxx, ax[c]), pminy = fmin(pminy, ay[c]), pmaxy = fmax(pmaxy, ay[c]);
        double tminx = bx[0], tmaxx = bx[0], tminy = by[0], tmaxy = by[0];
        for (int c = 1; c < 4; ++c) tminx = fmin(tminx, bx[c]), tmaxx = fmax(tmaxx, bx[c]), tminy = fmin(tminy, by[c]), tmaxy = fmax(tmaxy, by[c]);
        double v = 0.0;
        if (pminx < tmaxx && tminx < pmaxx && pminy < tmaxy && tminy < pmaxy) {
            const double pa = area_of(ax, ay, 4), ta = area_of(bx, by, 4);
            if (pa != 0.0 && ta != 0.0) {
                const double inter = quad_inter(ax, ay, bx, by);
                if (inter > 0.0) {
                    v = inter / (pa + ta - inter);
                    if (gt_ignore[e.g0 + j] && inter / pa > 0.5) atomicOr(ign_hit + e.p0 + i, 1);
                }
            }
        }
        iou[e.m0 + k] = v;
    }
}

// Rounds of mutually-best pairs.  Among the free words of a round the first pair of the total order is mutually best, and a mutually-best pair
// is one the greedy loop takes (any pair ahead of it in the order shares an end with it and would be that end's best instead), so every round
// takes only pairs of the greedy matching and at least one while a candidate is left: the fixed point is the greedy matching itself.  A word
// keeps its best partner between rounds and looks again only when that partner was taken by someone else.
__global__ __launch_bounds__(256) void k_ev_match(const double* __restrict__ iou, const long long* __restrict__ pair_offs, const int* __restrict__ pred_offs,
                                                  const int* __restrict__ gt_offs, const unsigned char* __restrict__ gt_ignore,
                                                  const int* __restrict__ ign_hit, long P, long G, long n_pairs, double min_iou, int* gt_of_pred,
                                                  int* pred_of_gt, double* __restrict__ iou_of_pred, int* bestg, int* bestp) {
    __shared__ int s_any;
    const EvPage e = ev_page(pred_offs, gt_offs, pair_offs, blockIdx.x, P, G, n_pairs);
    if (!e.ok) return;
    const int np = (int)e.np, ng = (int)e.ng, t = threadIdx.x;
    const double* M = iou + e.m0;
    int* gop = gt_of_pred + e.p0;
    int* pog = pred_of_gt + e.g0;
    int* bg = bestg + e.p0;
    int* bp = bestp + e.g0;
    const unsigned char* ign = gt_ignore + e.g0;
    for (int i = t; i < np; i += 256) gop[i] = -1, bg[i] = -2, iou_of_pred[e.p0 + i] = 0.0;  // -2: not looked yet; -1: no candidate left
    for (int j = t; j < ng; j += 256) pog[j] = -1, bp[j] = -2;
    __syncthreads();
    for (;;) {
        if (t == 0) s_any = 0;
        for (int i = t; i < np; i += 256) {
            if (gop[i] != -1) continue;
            const int cur = bg[i];
            if (cur == -1 || (cur >= 0 && pog[cur] == -1)) continue;
            double best = 0.0;
            int bj = -1;
            for (int j = 0; j < ng; ++j) {
                const double v = M[(long)i * ng + j];
                if (!ign[j] && pog[j] == -1 && v > min_iou && (bj < 0 || v > best)) best = v, bj = j;
            }
            bg[i] = bj;
        }
        for (int j = t; j < ng; j += 256) {
            if (pog[j] != -1 || ign[j]) continue;
            const int cur = bp[j];
            if (cur == -1 || (cur >= 0 && gop[cur] == -1)) continue;
            double best = 0.0;
            int bi = -1;
            for (int i = 0; i < np; ++i) {
                const double v = M[(long)i * ng + j];
                if (gop[i] == -1 && v > min_iou && (bi < 0 || v > best)) best = v, bi = i;
            }
            bp[j] = bi;
        }
        __syncthreads();
        for (int i = t; i < np; i += 256) {
            if (gop[i] != -1) continue;
            const int j = bg[i];
            if (j >= 0 && bp[j] == i) {
                gop[i] = j;
                pog[j] = i;
                iou_of_pred[e.p0 + i] = M[(long)i * ng + j];
                s_any = 1;
            }
        }
        __syncthreads();
        const int any = s_any;
        __syncthreads();
        if (!any) break;
    }
    for (int i = t; i < np; i += 256)
        if (gop[i] == -1 && ign_hit[e.p0 + i]) gop[i] = -2;
}

__device__ __forceinline__ int fold_ascii(int c) { return c >= 'A' && c <= 'Z' ? c + ('a' - 'A') : c; }
__device__ __forceinline__ void add64(long long* state, int k, long long v) {
    if (v) atomicAdd(reinterpret_cast<unsigned long long*>(state) + k, (unsigned long long)v);
}

// counters (int64[12]): 0 pages | 1 predictions not ignored | 2 annotations not ignored | 3 predictions ignored | 4 matched pairs | 5 exact |
// 6 exact ignoring ASCII case | 7 edit distance over matched pairs | 8 annotated characters of matched pairs | 9 predicted characters of
// unmatched, not ignored predictions | 10 annotated characters of unmatched, not ignored annotations | 11 annotated characters of all not
// ignored annotations
__global__ __launch_bounds__(64) void k_ev_text(const int* __restrict__ pred_offs, const int* __restrict__ gt_offs, long P, long G,
                                                const int* __restrict__ gt_of_pred, const int* pred_text, const int* __restrict__ pred_text_offs,
                                                long n_pred_text, const int* gt_text, const int* __restrict__ gt_text_offs, long n_gt_text, int* bnd,
                                                int* __restrict__ dist, int* __restrict__ flags, long long* state) {
    const int b = blockIdx.y, lane = threadIdx.x;
    const long p0 = pred_offs[b], np = (long)pred_offs[b + 1] - p0, g0 = gt_offs[b], ng = (long)gt_offs[b + 1] - g0;
    if (p0 < 0 || np < 0 || p0 + np > P || g0 < 0 || ng < 0 || g0 + ng > G || blockIdx.x >= np) return;
    const long i = p0 + blockIdx.x;
    const long a0 = pred_text_offs[i];
    const int m = __builtin_amdgcn_readfirstlane((int)(pred_text_offs[i + 1] - a0));
    const int j = __builtin_amdgcn_readfirstlane(gt_of_pred[i]);
    int d = -1, fl = 0;
    if (a0 < 0 || m < 0 || a0 + m > n_pred_text) return;
    if (j >= 0 && j < ng) {
        const long c0 = gt_text_offs[g0 + j];
        const int n = __builtin_amdgcn_readfirstlane((int)(gt_text_offs[g0 + j + 1] - c0));
        if (c0 < 0 || n < 0 || c0 + n > n_gt_text) return;
        const int* a = pred_text + a0;
        const int* c = gt_text + c0;
        d = wave_edit_distance(a, m, c, n, nullptr, 0, bnd + a0, lane);
        bool ne = m != n, nf = m != n;
        if (m == n)
            for (int k0 = 0; k0 < m; k0 += 64) {
                const int k = k0 + lane;
                const int x = k < m ? a[k] : 0, y = k < m ? c[k] : 0;
                ne |= __ballot(x != y) != 0ull;
                nf |= __ballot(fold_ascii(x) != fold_ascii(y)) != 0ull;
            }
        fl = (ne ? 0 : 1) | (nf ? 0 : 2);
        if (lane == 0 && state) {
            add64(state, 1, 1), add64(state, 4, 1), add64(state, 5, fl & 1), add64(state, 6, fl >> 1);
            add64(state, 7, d), add64(state, 8, n);
        }
    } else if (lane == 0 && state) {
        if (j == -2)
            add64(state, 3, 1);
        else
            add64(state, 1, 1), add64(state, 9, m);
    }
    if (lane == 0) dist[i] = d, flags[i] = fl;
}

__global__ __launch_bounds__(256) void k_ev_truth(long G, const unsigned char* __restrict__ gt_ignore, const int* __restrict__ pred_of_gt,
                                                  const int* __restrict__ gt_text_offs, int B, long long* state) {
    long long cnt = 0, all = 0, miss = 0;
    for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < G; j += (long)gridDim.x * 256) {
        if (gt_ignore[j]) continue;
        const long long n = (long long)gt_text_offs[j + 1] - gt_text_offs[j];
        cnt += 1, all += n, miss += pred_of_gt[j] < 0 ? n : 0;
    }
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o), all += __shfl_down(all, o), miss += __shfl_down(miss, o);
    if ((threadIdx.x & 63) == 0) add64(state, 2, cnt), add64(state, 11, all), add64(state, 10, miss);
    if (blockIdx.x == 0 && threadIdx.x == 0) add64(state, 0, B);
}

constexpr long EV_MAX = (1L << 31) - 2;  // pooled indices stay 32-bit

}  // namespace

extern "C" {

long ocrs_eval_match_ws_bytes(long P, long G) { return P < 0 || G < 0 || P > EV_MAX || G > EV_MAX ? 0 : (P + G + 1) * 4; }

int ocrs_eval_pair_iou(const float* pred_quads, const int* pred_offs, const float* gt_quads, const int* gt_offs, const unsigned char* gt_ignore,
                       const long long* pair_offs, int B, long P, long G, long n_pairs, long max_pairs, double* iou, int* ign_hit, hipStream_t st) {
    OCRS_CHECK_ARG(B >= 0 && B <= 65535 && P >= 0 && G >= 0 && P <= EV_MAX && G <= EV_MAX && n_pairs >= 0 && max_pairs >= 0 && max_pairs <= n_pairs);
    if (P > 0) {
        OCRS_CHECK_ARG(ign_hit);
        if (hipMemsetAsync(ign_hit, 0, (size_t)P * 4, st) != hipSuccess) return OCRS_ERR_HIP;
    }
    if (B == 0 || max_pairs == 0) return OCRS_OK;
    OCRS_CHECK_ARG(pred_quads && pred_offs && gt_quads && gt_offs && gt_ignore && pair_offs && iou);
    const long gx = (max_pairs + 255) / 256;
    hipLaunchKernelGGL(k_ev_pairs, dim3((unsigned)(gx < 4096 ? gx : 4096), B), dim3(256), 0, st, pred_quads, pred_offs, gt_quads, gt_offs, gt_ignore,
                       pair_offs, P, G, n_pairs, iou, ign_hit);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

int ocrs_eval_match(const double* iou, const long long* pair_offs, const int* pred_offs, const int* gt_offs, const unsigned char* gt_ignore,
                    const int* ign_hit, int B, long P, long G, long n_pairs, double min_iou, int* gt_of_pred, int* pred_of_gt, double* iou_of_pred, void* ws,
                    hipStream_t st) {
    OCRS_CHECK_ARG(B >= 0 && P >= 0 && G >= 0 && P <= EV_MAX && G <= EV_MAX && n_pairs >= 0);
    if (B == 0) return OCRS_OK;
    OCRS_CHECK_ARG(pair_offs && pred_offs && gt_offs && ws && (P == 0 || (ign_hit && gt_of_pred && iou_of_pred)) && (G == 0 || (gt_ignore && pred_of_gt)) &&
                   (n_pairs == 0 || iou));
    int* bestg = static_cast<int*>(ws);
    hipLaunchKernelGGL(k_ev_match, dim3(B), dim3(256), 0, st, iou, pair_offs, pred_offs, gt_offs, gt_ignore, ign_hit, P, G, n_pairs, min_iou, gt_of_pred,
                       pred_of_gt, iou_of_pred, bestg, bestg + P);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

int ocrs_eval_text_update(const int* pred_offs, const int* gt_offs, const unsigned char* gt_ignore, int B, long P, long G, int max_page_preds,
                          const int* gt_of_pred, const int* pred_of_gt, const int* pred_text, const int* pred_text_offs, long n_pred_text,
                          const int* gt_text, const int* gt_text_offs, long n_gt_text, int* bnd, int* dist, int* flags, long long* state, hipStream_t st) {
    OCRS_CHECK_ARG(B >= 0 && B <= 65535 && P >= 0 && G >= 0 && P <= EV_MAX && G <= EV_MAX && max_page_preds >= 0 && max_page_preds <= P && n_pred_text >= 0 &&
                   n_gt_text >= 0);
    if (B == 0) return OCRS_OK;
    OCRS_CHECK_ARG(pred_offs && gt_offs);
    if (P > 0 && max_page_preds > 0) {
        OCRS_CHECK_ARG(gt_of_pred && pred_text_offs && dist && flags && (n_pred_text == 0 || (pred_text && bnd)) && (G == 0 || gt_text_offs) &&
                       (n_gt_text == 0 || gt_text));
        hipLaunchKernelGGL(k_ev_text, dim3(max_page_preds, B), dim3(64), 0, st, pred_offs, gt_offs, P, G, gt_of_pred, pred_text, pred_text_offs, n_pred_text,
                           gt_text, gt_text_offs, n_gt_text, bnd, dist, flags, state);
    }
    if (state) {
        OCRS_CHECK_ARG(G == 0 || (gt_ignore && pred_of_gt && gt_text_offs));
        const long gx = (G + 255) / 256;
        hipLaunchKernelGGL(k_ev_truth, dim3((unsigned)(gx < 1 ? 1 : (gx < 1024 ? gx : 1024))), dim3(256), 0, st, G, gt_ignore, pred_of_gt, gt_text_offs, B, state);
    }
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

}  // extern "C"
