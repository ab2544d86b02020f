// Layout training data (ocrs_models/datasets/web_layout.py:76-186): one batch of WebLayout items assembled on the device from the
// parsed dataset, which lives in HBM (fp64 word coordinates of every page, parsed once; Python: ocrs_models_amd/datasets.py).
//   k_weblayout_batch   one lane per (page of the batch, word slot): jitter, optional normalisation, the one fp64 -> fp32 rounding of
//                       torch.Tensor(words), the line_start / line_end labels from the word's paragraph neighbours, zero padding
// The reference computes on Python floats, so every operation here is a single IEEE fp64 operation (no contraction, no reciprocal) and
// the result is bit-identical to it.  Every lane stores unconditionally (16 + 8 bytes); no atomics, nothing synchronises.
#include "common.h"

#pragma clang fp contract(off)

namespace {

// transform() of web_layout.py:113-132 on one coordinate: c * scale + jitter with scale = 1.0, then c / viewport - 0.5
__device__ __forceinline__ double wl_coord(double c, double jitter, double viewport, int normalize) {
    c = c * 1.0 + jitter;
    if (normalize) c = c / viewport - 0.5;
    return c;
}

// intervals_overlap (datasets/util.py:197-204): asymmetric on purpose, touching intervals do not overlap
__device__ __forceinline__ bool wl_overlap(double a, double b, double c, double d) { return a <= c ? b > c : d > a; }

__global__ __launch_bounds__(256) void k_weblayout_batch(const double* __restrict__ coords, const int* __restrict__ para,
                                                         const long long* __restrict__ page_off, const double* __restrict__ viewport,
                                                         const int* __restrict__ pages, const double* __restrict__ jitter, int N, int W, int P,
                                                         int normalize, float4* __restrict__ boxes, float2* __restrict__ labels) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < (long)N * W) {
        const int n = (int)(i / W), w = (int)(i - (long)n * W);
        int page = pages[n];
        page = page < 0 ? 0 : (page >= P ? P - 1 : page);  // (indices are checked on the host; never read outside the dataset)
        const long long lo = page_off[page], cnt = page_off[page + 1] - lo;
        float4 bx = make_float4(0.f, 0.f, 0.f, 0.f);
        float2 lb = make_float2(0.f, 0.f);
        if (w < cnt) {
            const double jx = jitter[2 * n], jy = jitter[2 * n + 1];
            const double vw = viewport[2 * page], vh = viewport[2 * page + 1];
            const long long t = lo + w;
            const double* c = coords + 4 * t;
            const double left = wl_coord(c[0], jx, vw, normalize), top = wl_coord(c[1], jy, vh, normalize);
            const double right = wl_coord(c[2], jx, vw, normalize), bottom = wl_coord(c[3], jy, vh, normalize);
            bx = make_float4((float)left, (float)top, (float)right, (float)bottom);
            const int pa = para[t];
            // the neighbours are words of the PAGE, not of the padded row: slot W - 1 looks at word W (truncation comes after labelling)
            bool start = true, end = true;
            if (w > 0 && para[t - 1] == pa) {
                const double pt = wl_coord(c[-3], jy, vh, normalize), pb = wl_coord(c[-1], jy, vh, normalize);
                start = !wl_overlap(pt, pb, top, bottom);
            }
            if (w + 1 < cnt && para[t + 1] == pa) {
                const double nt = wl_coord(c[5], jy, vh, normalize), nb = wl_coord(c[7], jy, vh, normalize);
                end = !wl_overlap(top, bottom, nt, nb);
            }
            lb = make_float2(start ? 1.f : 0.f, end ? 1.f : 0.f);
        }
        boxes[i] = bx;
        labels[i] = lb;
    }
}

}  // namespace

extern "C" {

int ocrs_weblayout_batch(const double* coords, const int* para, const long long* page_off, const double* viewport, int P, const int* pages,
                         const double* jitter, int N, int W, int normalize, float* boxes, float* labels, hipStream_t st) {
    OCRS_CHECK_ARG(coords && para && page_off && viewport && pages && jitter && boxes && labels && P >= 1 && N >= 1 && W >= 1 &&
                   (reinterpret_cast<uintptr_t>(boxes) & 15) == 0 && (reinterpret_cast<uintptr_t>(labels) & 7) == 0);
    const long nb = ((long)N * W + 255) / 256;
    OCRS_CHECK_ARG(nb <= 0x7fffffffL);
    hipLaunchKernelGGL(k_weblayout_batch, dim3((int)nb), dim3(256), 0, st, coords, para, page_off, viewport, pages, jitter, N, W, P, normalize,
                       reinterpret_cast<float4*>(boxes), reinterpret_cast<float2*>(labels));
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

}  // extern "C"
