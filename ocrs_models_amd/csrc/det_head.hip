// Detection head out_conv (Conv2d 8 -> 1, 1x1, bias + Sigmoid; ocrs_models/models.py:125-129, 143), forward and backward (gfx950).
//
//  k_head_fwd        pred = sigmoid(w . relu(bn(z)) + b)
//  k_head_bwd        gy or gl = dL/dlogit, dw, db (+ the BatchNorm-backward sums of the block that produced z)
//  k_head_bwd_loss   the same with the balanced-BCE backward fused in: dL/dpred formed on the fly from the loss forward's saved state
#include "det_common.h"
#include "loss_state.h"

// out_conv: Conv2d(8 -> 1, 1x1, bias) + Sigmoid (models.py:125-129) on relu(bn(z)).  pred is fp32 (B,1,H,W).
template <class T>
__global__ __launch_bounds__(256) void k_head_fwd(const T* __restrict__ z, const float* __restrict__ tr, const float* __restrict__ w,
                                                  const float* __restrict__ b, float* __restrict__ pred, long P) {
    float wv[8], sc[8], sh[8], lo[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        wv[i] = w[i];
        sc[i] = tr[i];
        sh[i] = tr[8 + i];
        lo[i] = tr[16 + i];
    }
    const float bias = b[0];
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < P; p += (long)gridDim.x * 256) {
        float v[8];
        load8(z + p * 8, v);
        float s = bias;
#pragma unroll
        for (int i = 0; i < 8; ++i) s = fmaf(wv[i], fmaxf(fmaf(v[i], sc[i], sh[i]), lo[i]), s);
        pred[p] = 1.f / (1.f + __expf(-s));
    }
}

// head backward: pred = sigmoid(w . x~ + b);  gl = gpred * pred * (1 - pred);  gy[p][c] = gl * w[c];  dw, db.
template <class T>
__global__ __launch_bounds__(256) void k_head_bwd(const T* __restrict__ z, const float* __restrict__ tr, const float* __restrict__ w,
                                                  const float* __restrict__ pred, const float* __restrict__ gpred, T* __restrict__ gy,
                                                  double* __restrict__ acc64 /*[9]: dw[8] | db*/, const float* __restrict__ saved /*[2][8] or null*/,
                                                  double* __restrict__ gsum /*[2][8] or null*/, long P, float* __restrict__ gl_out /*[P] or null*/) {
    // gl_out != null (round 5): instead of the 8-channel gradient gy (16 B per pixel in bf16) only gl = dL/dlogit is written (4 B); the block
    // backward that consumes it (k_rs_bwd<..., HEAD>) forms gy = round(gl * w[c]) on the fly -- the same values: 12 B per pixel less written here
    // and 12 B less read there
    // gsum != null: also the BatchNorm-backward sums (sum ghat, sum ghat*zhat) of the block that produced z -- this kernel is that
    // block's only consumer and already reads z, so its k_bn_bwd_reduce pass (0.24 ms at 32x1024^2) is not needed
    __shared__ float s_slots[4 * 25];
    float wv[8], sc[8], sh[8], lo[8], mu[8], acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, st1[8], st2[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        wv[i] = w[i];
        sc[i] = tr[i];
        sh[i] = tr[8 + i];
        lo[i] = tr[16 + i];
        mu[i] = gsum ? saved[i] : 0.f;
        st1[i] = st2[i] = 0.f;
    }
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < P; p += (long)gridDim.x * 256) {
        const float pr = pred[p];
        const float gl = gpred[p] * (1.f - pr) * pr;
        float v[8], o[8];
        load8(z + p * 8, v);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float pre = fmaf(v[i], sc[i], sh[i]);
            const float xv = fmaxf(pre, lo[i]);
            acc[i] = fmaf(gl, xv, acc[i]);
            o[i] = gl * wv[i];
            const float gh = pre > 0.f ? Elem<T>::round(o[i]) : 0.f;  // what the block's pw_bwd will read back
            st1[i] += gh;
            st2[i] = fmaf(gh, v[i] - mu[i], st2[i]);
        }
        acc[8] += gl;
        if (gl_out) gl_out[p] = gl;
        else store8(gy + p * 8, o);
    }
    // deterministic block sums (no LDS float atomics), fp64 accumulation across blocks
    float all[25];
#pragma unroll
    for (int i = 0; i < 9; ++i) all[i] = acc[i];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        all[9 + i] = st1[i];
        all[17 + i] = st2[i];
    }
    const float tot = block_sum_det<25>(all, s_slots);
    if (threadIdx.x < 9) atomicAdd(&acc64[threadIdx.x], (double)tot);
    if (gsum && threadIdx.x >= 9 && threadIdx.x < 25) {
        const int i = threadIdx.x - 9;  // 0..7: sum ghat, 8..15: sum ghat*(z - mean) -> * rstd
        atomicAdd(&gsum[i], (double)(i < 8 ? tot : tot * saved[8 + (i - 8)]));
    }
}

// Balanced-BCE backward + head backward in ONE pass (round 5): dL/dpred is formed on the fly from what the loss forward saved (class map,
// per-pixel loss, the two radix-select thresholds: the arithmetic of k_bce_bwd in loss_optim.hip, operation for operation) instead of being
// written by k_bce_bwd (4 B per pixel) and read back here (4 B) -- 33 instead of 45 B per pixel over the two launches, one launch and one
// 134 MB buffer less per step.  Four pixels per thread and iteration (16-byte loads of pred / target / lpx, one dword of classes, four 16-byte z
// vectors, one 16-byte gl store).  Only the gl form (k_rs_bwd<..., HEAD> consumes gl); P % 4 == 0.
template <class T>
__global__ __launch_bounds__(256) void k_head_bwd_loss(const T* __restrict__ z, const float* __restrict__ tr, const float* __restrict__ w,
                                                       const float* __restrict__ pred, const float* __restrict__ target,
                                                       const float* __restrict__ lpx, const unsigned char* __restrict__ cls,
                                                       const LossState* __restrict__ stt, const float* __restrict__ gout,
                                                       double* __restrict__ acc64 /*[9]: dw[8] | db*/, const float* __restrict__ saved /*[2][8]*/,
                                                       double* __restrict__ gsum /*[2][8]*/, long P, float* __restrict__ gl_out /*[P]*/) {
    __shared__ float s_slots[4 * 25];
    float wv[8], sc[8], sh[8], lo[8], mu[8], acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, st1[8], st2[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        wv[i] = w[i];
        sc[i] = tr[i];
        sh[i] = tr[8 + i];
        lo[i] = tr[16 + i];
        mu[i] = saved[i];
        st1[i] = st2[i] = 0.f;
    }
    const unsigned t0 = stt->prefix[0], t1 = stt->prefix[1];
    const float f0 = stt->frac[0], f1 = stt->frac[1];
    const float s = gout[0] * stt->inv2k;
    const long nq = P >> 2;
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < nq; q += (long)gridDim.x * 256) {
        const float4 p4 = reinterpret_cast<const float4*>(pred)[q], t4 = reinterpret_cast<const float4*>(target)[q];
        const float4 l4 = reinterpret_cast<const float4*>(lpx)[q];
        const unsigned c4 = reinterpret_cast<const unsigned*>(cls)[q];
        float v[4][8];
#pragma unroll
        for (int e = 0; e < 4; ++e) load8(z + (q * 4 + e) * 8, v[e]);
        const float pe[4] = {p4.x, p4.y, p4.z, p4.w}, te[4] = {t4.x, t4.y, t4.z, t4.w}, le[4] = {l4.x, l4.y, l4.z, l4.w};
        float gle[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const unsigned c = (c4 >> (8 * e)) & 0xffu;
            const float pr = pe[e];
            float gp = 0.f;  // k_bce_bwd's grad()
            if (c) {
                const unsigned key = loss_key(le[e]);
                const unsigned thr = c == 1 ? t0 : t1;
                const float wgt = key > thr ? 1.f : (key == thr ? (c == 1 ? f0 : f1) : 0.f);
                if (wgt != 0.f) {
                    const float t = fminf(fmaxf(te[e], 0.f), 1.f);
                    gp = s * wgt * (pr - t) / fmaxf((1.f - pr) * pr, 1e-12f);
                }
            }
            const float gl = gp * (1.f - pr) * pr;
            gle[e] = gl;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float pre = fmaf(v[e][i], sc[i], sh[i]);
                const float xv = fmaxf(pre, lo[i]);
                acc[i] = fmaf(gl, xv, acc[i]);
                const float gh = pre > 0.f ? Elem<T>::round(gl * wv[i]) : 0.f;  // what the block's backward forms from gl
                st1[i] += gh;
                st2[i] = fmaf(gh, v[e][i] - mu[i], st2[i]);
            }
            acc[8] += gl;
        }
        reinterpret_cast<float4*>(gl_out)[q] = make_float4(gle[0], gle[1], gle[2], gle[3]);
    }
    float all[25];
#pragma unroll
    for (int i = 0; i < 9; ++i) all[i] = acc[i];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        all[9 + i] = st1[i];
        all[17 + i] = st2[i];
    }
    const float tot = block_sum_det<25>(all, s_slots);
    if (threadIdx.x < 9) atomicAdd(&acc64[threadIdx.x], (double)tot);
    if (threadIdx.x >= 9 && threadIdx.x < 25) {
        const int i = threadIdx.x - 9;
        atomicAdd(&gsum[i], (double)(i < 8 ? tot : tot * saved[8 + (i - 8)]));
    }
}

// ----------------------------------------------------------------------------------------------
// host side
// ----------------------------------------------------------------------------------------------
// Head backward: gy [P][8] written (dtype T); acc64 [9] fp64 = dw [8] | db, ACCUMULATED (caller-zeroed, caller adds it to the fp32 gradients).  saved / gsum (nullable): also accumulate the BatchNorm-backward
// sums [2][8] (fp64, caller-zeroed) of the block that produced z (saved = its [mean | rstd]) -- replaces that block's ocrs_bn_bwd_reduce.
static int head_bwd_impl(const void* z, const float* tr, const float* w, const float* pred, const float* gpred, void* gy, float* gl, double* acc64,
                         const float* saved, double* gsum, long P, int dtype, hipStream_t st) {
    OCRS_CHECK_ARG(z && tr && w && pred && gpred && (gy || gl) && acc64 && P > 0 && (!gsum || saved));
    int grid = ew_grid(P);
    if (grid > 1024) grid = 1024;  // streaming kernel ending in same-address atomics: 4 blocks per CU are plenty
    if (dtype == 1)
        hipLaunchKernelGGL(k_head_bwd<bf16>, dim3(grid), dim3(256), 0, st, (const bf16*)z, tr, w, pred, gpred, (bf16*)gy, acc64, saved, gsum, P, gl);
    else
        hipLaunchKernelGGL(k_head_bwd<float>, dim3(grid), dim3(256), 0, st, (const float*)z, tr, w, pred, gpred, (float*)gy, acc64, saved, gsum, P, gl);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

// ----------------------------------------------------------------------------------------------
// C ABI
// ----------------------------------------------------------------------------------------------
extern "C" {

// out_conv 1x1 (8->1) + bias + sigmoid (models.py:125-129).  pred fp32 [N][1][H][W].
int ocrs_head_fwd(const void* z, const float* tr, const float* w, const float* b, float* pred, long P, int dtype, hipStream_t st) {
    OCRS_CHECK_ARG(z && tr && w && b && pred && P > 0);
    const int grid = ew_grid(P);
    if (dtype == 1)
        hipLaunchKernelGGL(k_head_fwd<bf16>, dim3(grid), dim3(256), 0, st, (const bf16*)z, tr, w, b, pred, P);
    else
        hipLaunchKernelGGL(k_head_fwd<float>, dim3(grid), dim3(256), 0, st, (const float*)z, tr, w, b, pred, P);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

int ocrs_head_bwd(const void* z, const float* tr, const float* w, const float* pred, const float* gpred, void* gy, double* acc64,
                  const float* saved, double* gsum, long P, int dtype, hipStream_t st) {
    OCRS_CHECK_ARG(gy);
    return head_bwd_impl(z, tr, w, pred, gpred, gy, nullptr, acc64, saved, gsum, P, dtype, st);
}
// ocrs_head_bwd that writes gl [P] fp32 = dL/dlogit instead of the 8-channel gradient gy: for ocrs_mm_bwd_fin_head, which forms gy on the fly
int ocrs_head_bwd_gl(const void* z, const float* tr, const float* w, const float* pred, const float* gpred, float* gl, double* acc64,
                     const float* saved, double* gsum, long P, int dtype, hipStream_t st) {
    OCRS_CHECK_ARG(gl);
    return head_bwd_impl(z, tr, w, pred, gpred, nullptr, gl, acc64, saved, gsum, P, dtype, st);
}
// ocrs_balanced_bce_bwd + ocrs_head_bwd_gl in one pass: dL/dpred is formed on the fly from the loss forward's saved tensors (pred, target, lpx, cls,
// state: ocrs_balanced_bce_fwd) and gout [1] (the upstream gradient of the scalar loss) -- reference: the autograd of train_detection.py:225-263
// followed by models.py:143's 1x1 conv + sigmoid backward.  P % 4 == 0, saved / gsum required.
int ocrs_head_bwd_loss(const void* z, const float* tr, const float* w, const float* pred, const float* target, const float* lpx, const unsigned char* cls,
                       const void* state, const float* gout, float* gl, double* acc64, const float* saved, double* gsum, long P, int dtype,
                       hipStream_t st) {
    OCRS_CHECK_ARG(z && tr && w && pred && target && lpx && cls && state && gout && gl && acc64 && saved && gsum && P > 0 && P % 4 == 0);
    int grid = ew_grid(P / 4);  // (ew_grid caps at 8 blocks per CU)
    if (dtype == 1)
        hipLaunchKernelGGL(k_head_bwd_loss<bf16>, dim3(grid), dim3(256), 0, st, (const bf16*)z, tr, w, pred, target, lpx, cls, (const LossState*)state,
                           gout, acc64, saved, gsum, P, gl);
    else
        hipLaunchKernelGGL(k_head_bwd_loss<float>, dim3(grid), dim3(256), 0, st, (const float*)z, tr, w, pred, target, lpx, cls,
                           (const LossState*)state, gout, acc64, saved, gsum, P, gl);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

}  // extern "C"
