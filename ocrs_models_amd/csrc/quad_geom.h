// fp64 geometry of convex quads that repeats the host's arithmetic operation by operation (ocrs_models_amd/postprocess.py: _area, _ccw, _clip,
// quad_intersection_area): shared by the box match of the validation metrics (postprocess.hip) and the pair IoU of the end-to-end accuracy
// (ocr_eval.hip).  Where the host itself fuses (numpy's dot goes through BLAS, whose kernels use fma) the same fma is written out; everything
// else must not be contracted, so FMA contraction is off from here on in every file that includes this header.
#pragma once
#include "common.h"

#pragma clang fp contract(off)

namespace {

// np.dot(u, roll(v, -1)) of the host on the stride-2 columns of an (n, 2) array: BLAS ddot's strided loop -- two partial sums over groups of
// four (each adding fma(u0, v0, u2 * v2) resp. fma(u1, v1, u3 * v3)), a fused tail into the first, then their sum
__device__ __forceinline__ double host_dot_rolled(const double* u, const double* v, int n) {
    auto vr = [&](int i) { return v[i + 1 == n ? 0 : i + 1]; };
    double t1 = 0.0, t2 = 0.0;
    int i = 0;
    for (; i + 4 <= n; i += 4) {
        t1 = t1 + fma(vr(i), u[i], vr(i + 2) * u[i + 2]);
        t2 = t2 + fma(vr(i + 1), u[i + 1], vr(i + 3) * u[i + 3]);
    }
    for (; i < n; ++i) t1 = fma(vr(i), u[i], t1);
    return t1 + t2;
}
// the signed shoelace sum of _area / _ccw: x . roll(y, -1) - y . roll(x, -1)
__device__ __forceinline__ double shoelace2(const double* x, const double* y, int n) { return host_dot_rolled(x, y, n) - host_dot_rolled(y, x, n); }
__device__ __forceinline__ double area_of(const double* x, const double* y, int n) { return n < 3 ? 0.0 : 0.5 * fabs(shoelace2(x, y, n)); }

constexpr int MAXV = 16;  // clip output: a convex 4-gon clipped by 4 half-planes has at most 8 vertices

// quad_intersection_area of the host: Sutherland-Hodgman of ccw(a) by ccw(b), then the shoelace area
__device__ double quad_inter(const double* ax, const double* ay, const double* bx, const double* by) {
    double sx[MAXV], sy[MAXV], ox[MAXV], oy[MAXV], cx[4], cy[4];
    const bool fa = shoelace2(ax, ay, 4) < 0, fb = shoelace2(bx, by, 4) < 0;
    for (int i = 0; i < 4; ++i) {
        ox[i] = ax[fa ? 3 - i : i], oy[i] = ay[fa ? 3 - i : i];
        cx[i] = bx[fb ? 3 - i : i], cy[i] = by[fb ? 3 - i : i];
    }
    int n = 4;
    for (int e = 0; e < 4; ++e) {
        if (n == 0) break;
        const double ex0 = cx[e], ey0 = cy[e], ex1 = cx[(e + 1) & 3], ey1 = cy[(e + 1) & 3];
        for (int j = 0; j < n; ++j) sx[j] = ox[j], sy[j] = oy[j];
        const int m = n;
        n = 0;
        for (int j = 0; j < m; ++j) {
            const int j1 = j + 1 == m ? 0 : j + 1;
            const double sp = (ex1 - ex0) * (sy[j] - ey0) - (ey1 - ey0) * (sx[j] - ex0);
            const double sq = (ex1 - ex0) * (sy[j1] - ey0) - (ey1 - ey0) * (sx[j1] - ex0);
            if (sp >= 0 && n < MAXV) ox[n] = sx[j], oy[n] = sy[j], ++n;
            if (((sp > 0 && sq < 0) || (sp < 0 && sq > 0)) && n < MAXV) {
                const double t = sp / (sp - sq);
                ox[n] = sx[j] + t * (sx[j1] - sx[j]);
                oy[n] = sy[j] + t * (sy[j1] - sy[j]);
                ++n;
            }
        }
    }
    return area_of(ox, oy, n);
}

__device__ __forceinline__ void load_quad(const float* q, double* x, double* y) {
    for (int i = 0; i < 4; ++i) x[i] = (double)q[2 * i], y[i] = (double)q[2 * i + 1];
}

}  // namespace
