// Training augmentations of the two train loops on the device: the reference's host-side torchvision pipelines,
// batched over variable-size samples.
//
//   k_aug_*_stats   ColorJitter's contrast mean   torchvision adjust_contrast: per-image mean, fixed summation order, no atomics
//   k_aug_det       prepare_transform(mask_size)  ocrs_models/train_detection.py:266-290: RandomApply(RandomChoice([ColorJitter,
//                                                 RandomAffine, RandomPerspective, RandomCrop])) + Resize(mask_size, antialias=False),
//                                                 fused: no intermediate image is materialised
//   k_aug_line_warp text_recognition_data_augmentations  ocrs_models/datasets/__init__.py:4-30 + hiertext.py:271-284 (background mask,
//                                                 RandomApply(RandomChoice([ColorJitter, RandomRotation(expand), Pad])), clamp)
//   k_aug_line_h/v  resize(.., antialias=True) + collate_samples' padding (hiertext.py:288-294, train_rec.py:285-299)
//
// The random parameters are drawn on the host (ocrs_models_amd/augment.py) and arrive as one record of kAugRec 32-bit words per sample;
// the sample index is blockIdx.z, so every record field is uniform over a workgroup.  The arithmetic restates torchvision's tensor path on
// ATen's CPU kernels operation by operation, with the FMAs ATen's CPU build contracts made explicit (fmaf) and no other contraction.
#include "input_pipe.h"

namespace {

constexpr int kAugRec = 24;  // words per sample record, see ocrs_hip.h
enum : int { kIdentity = 0, kJitter = 1, kAffineNearest = 2, kPerspective = 3, kShift = 4, kAffineBilinear = 5 };

struct Rec {
    int kind, flags, h, w, ih, iw, dy, dx, ow;
    float f[8];
};
__device__ __forceinline__ Rec load_rec(const int* p) {
    Rec r;
    r.kind = p[0], r.flags = p[1], r.h = p[2], r.w = p[3], r.ih = p[4], r.iw = p[5], r.dy = p[6], r.dx = p[7], r.ow = p[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) r.f[i] = __int_as_float(p[16 + i]);
    return r;
}

// Where intermediate pixel (y, x) comes from in the source: one element (i[0], -1 = outside: the fill value) or, for the bilinear warps,
// four corners (-1 = outside: zero padding) with grid_sample's weights and the coverage m of the ones channel.
struct Gather {
    int i[4];
    float w[4];
    float m;
};

__device__ __forceinline__ int src_index(const Rec& r, int y, int x) { return (y >= 0 && y < r.h && x >= 0 && x < r.w) ? y * r.w + x : -1; }

// _gen_affine_grid / _perspective_grid: base_grid.bmm(theta), a K=3 product, in the unfused order (x * t0 + y * t1) + t2 (CPU GEMMs
// differ here by an ulp; tests/augment_ref.py fixes this order).
__device__ __forceinline__ void grid_at(const Rec& r, int y, int x, float& gx, float& gy) {
#pragma clang fp contract(off)
    if (r.kind == kPerspective) {
        const float bx = (float)x + 0.5f, by = (float)y + 0.5f;
        const float n0 = (bx * r.f[0] + by * r.f[1]) + r.f[2];
        const float n1 = (bx * r.f[3] + by * r.f[4]) + r.f[5];
        const float d = (bx * r.f[6] + by * r.f[7]) + 1.0f;
        gx = n0 / d - 1.0f;
        gy = n1 / d - 1.0f;
    } else {
        const float bx = (float)x + r.f[6], by = (float)y + r.f[7];
        gx = (bx * r.f[0] + by * r.f[1]) + r.f[2];
        gy = (bx * r.f[3] + by * r.f[4]) + r.f[5];
    }
}

// grid_sample(padding_mode="zeros", align_corners=False) on ATen's CPU kernel: unnormalise = (g + 1) * (size / 2) - 0.5 (one FMA).
__device__ __forceinline__ Gather locate(const Rec& r, int y, int x) {
#pragma clang fp contract(off)
    Gather g;
    g.i[1] = g.i[2] = g.i[3] = -1;
    g.w[0] = g.w[1] = g.w[2] = g.w[3] = 0.0f;
    g.m = 0.0f;
    if (r.kind == kIdentity || r.kind == kJitter) {
        g.i[0] = src_index(r, y, x);
    } else if (r.kind == kShift) {
        g.i[0] = src_index(r, y + r.dy, x + r.dx);
    } else {
        float gx, gy;
        grid_at(r, y, x, gx, gy);
        const float ix = fmaf(gx + 1.0f, 0.5f * (float)r.w, -0.5f), iy = fmaf(gy + 1.0f, 0.5f * (float)r.h, -0.5f);
        if (r.kind == kAffineNearest) {
            const float rx = rintf(ix), ry = rintf(iy);  // round half to even, as ATen's CPU nearest
            g.i[0] = (rx >= 0.0f && rx < (float)r.w && ry >= 0.0f && ry < (float)r.h) ? (int)ry * r.w + (int)rx : -1;
        } else {
            const float fx = floorf(ix), fy = floorf(iy);
            const float we = ix - fx, ee = 1.0f - we, ns = iy - fy, ss = 1.0f - ns;
            g.w[0] = ss * ee, g.w[1] = ss * we, g.w[2] = ns * ee, g.w[3] = ns * we;
            // clamp before the int conversion so a far-off coordinate cannot overflow; anything clamped is outside anyway
            const int x0 = (int)fminf(fmaxf(fx, -2.0f), (float)r.w + 1.0f), y0 = (int)fminf(fmaxf(fy, -2.0f), (float)r.h + 1.0f);
            g.i[0] = src_index(r, y0, x0), g.i[1] = src_index(r, y0, x0 + 1);
            g.i[2] = src_index(r, y0 + 1, x0), g.i[3] = src_index(r, y0 + 1, x0 + 1);
            float m = (g.i[0] >= 0 ? 1.0f : 0.0f) * g.w[0];
#pragma unroll
            for (int k = 1; k < 4; ++k) m = fmaf(g.i[k] >= 0 ? 1.0f : 0.0f, g.w[k], m);
            g.m = m;
        }
    }
    return g;
}

// ColorJitter(brightness=0.1, contrast=0.1): adjust_brightness = clamp(b * x, 0, 1); adjust_contrast = clamp(c * x + (1 - c) * mean, 0, 1),
// the second term precomputed per image by k_aug_stats (cofs).  flags bit 0: brightness runs first.
__device__ __forceinline__ float bright(const Rec& r, float v) { return fminf(fmaxf(r.f[0] * v, 0.0f), 1.0f); }
__device__ __forceinline__ float jitter(const Rec& r, float v, float cofs) {
#pragma clang fp contract(off)
    if (r.flags & 1) v = bright(r, v);
    v = fminf(fmaxf(r.f[1] * v + cofs, 0.0f), 1.0f);
    if (!(r.flags & 1)) v = bright(r, v);
    return v;
}

// Value of intermediate pixel g on one plane; Src::ld(i) reads source element i of that plane.
template <class Src>
__device__ __forceinline__ float sample(const Rec& r, const Gather& g, const Src& s, float fill, float cofs) {
#pragma clang fp contract(off)
    if (r.kind != kPerspective && r.kind != kAffineBilinear) {
        if (g.i[0] < 0) return fill;
        const float v = s.ld(g.i[0]);
        return r.kind == kJitter ? jitter(r, v, cofs) : v;
    }
    float v = (g.i[0] >= 0 ? s.ld(g.i[0]) : 0.0f) * g.w[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) v = fmaf(g.i[k] >= 0 ? s.ld(g.i[k]) : 0.0f, g.w[k], v);
    return v * g.m + (1.0f - g.m) * fill;  // _apply_grid_transform's blend with the ones channel
}

struct SrcU8 {
    const uint8_t* p;
    __device__ float ld(int i) const { return px_u8(p[i]); }
};
struct SrcMaskU8 {
    const uint8_t* p;
    __device__ float ld(int i) const { return (float)p[i]; }
};
struct SrcF32 {
    const float* p;
    __device__ float ld(int i) const { return p[i]; }
};
// hiertext.py:273-274, -0.5 * (1 - m) + x * m for a 0/1 mask m (exactly a select); m == nullptr: no masking
template <class Src>
struct SrcMasked {
    Src s;
    const uint8_t* m;
    __device__ float ld(int i) const { return (m == nullptr || m[i]) ? s.ld(i) : -0.5f; }
};

// Per-image contrast term (1 - c) * mean of the jitter samples' planes, reduced in a fixed order without atomics so the result is
// bit-reproducible: kStatChunks workgroups per (sample, plane) each sum one contiguous chunk into an fp64 partial (fixed thread / tree
// order), then k_aug_stats_fin adds the partials in chunk order.  Workgroups of other samples exit at once.
constexpr int kStatChunks = 64;

template <class Src>
__device__ void stats_chunk(const Rec& r, const Src& s, double* part) {
    __shared__ double red[256];
    const int n = r.h * r.w;
    const int lo = (int)((long long)n * blockIdx.x / kStatChunks), hi = (int)((long long)n * (blockIdx.x + 1) / kStatChunks);
    double acc = 0.0;
    for (int i = lo + (int)threadIdx.x; i < hi; i += 256) {
        const float v = s.ld(i);
        acc += (double)((r.flags & 1) ? bright(r, v) : v);
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) *part = red[0];
}

// part [B][planes][kStatChunks] -> stats [B][planes]
__global__ __launch_bounds__(256) void k_aug_stats_fin(const int* __restrict__ params, const double* __restrict__ part, float* __restrict__ stats,
                                                       int B, int planes) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= B * planes) return;
    const Rec r = load_rec(params + (size_t)(t / planes) * kAugRec);
    if (r.kind != kJitter) return;
    double sum = 0.0;
    for (int c = 0; c < kStatChunks; ++c) sum += part[(size_t)t * kStatChunks + c];
    const float mean = (float)(sum / (double)(r.h * r.w));
    stats[t] = r.f[2] * mean;
}

template <int MK>
__global__ __launch_bounds__(256) void k_aug_det_stats(const uint8_t* __restrict__ img, const void* __restrict__ mask, const long long* __restrict__ offs,
                                                       const int* __restrict__ params, double* __restrict__ part) {
    const int b = blockIdx.z;
    const Rec r = load_rec(params + (size_t)b * kAugRec);
    if (r.kind != kJitter) return;
    const long long o = offs[b];
    double* out = part + ((size_t)b * 2 + blockIdx.y) * kStatChunks + blockIdx.x;
    if (blockIdx.y == 0)
        stats_chunk(r, SrcU8{img + o}, out);
    else if (MK == 0)
        stats_chunk(r, SrcMaskU8{static_cast<const uint8_t*>(mask) + o}, out);
    else
        stats_chunk(r, SrcF32{static_cast<const float*>(mask) + o}, out);
}

// Resize(mask_size, antialias=False) = upsample_bilinear2d(align_corners=False) from the intermediate (ih, iw) grid, whose pixels are
// computed from the source on the fly.  One thread per output pixel of both planes; block 64 x 4.
struct Lin {
    int i0, i1;
    float l0, l1;
};
__device__ __forceinline__ Lin lin_taps(int o, int n_in, int n_out) {
#pragma clang fp contract(off)
    Lin t;
    const float scale = (float)n_in / (float)n_out;
    const float src = fmaxf(fmaf(scale, (float)o + 0.5f, -0.5f), 0.0f);
    t.i0 = (int)src;
    t.i1 = t.i0 + (t.i0 < n_in - 1 ? 1 : 0);
    t.l1 = src - (float)t.i0;
    t.l0 = 1.0f - t.l1;
    return t;
}

template <typename T, int MK>
__global__ __launch_bounds__(256) void k_aug_det(const uint8_t* __restrict__ img, const void* __restrict__ mask, const long long* __restrict__ offs,
                                                 const int* __restrict__ params, const float* __restrict__ stats, T* __restrict__ img_out,
                                                 float* __restrict__ mask_out, int OH, int OW) {
#pragma clang fp contract(off)
    const int b = blockIdx.z;
    const int ox = blockIdx.x * 64 + threadIdx.x, oy = blockIdx.y * 4 + threadIdx.y;
    if (ox >= OW || oy >= OH) return;
    const Rec r = load_rec(params + (size_t)b * kAugRec);
    const long long o = offs[b];
    const SrcU8 si{img + o};
    const float c0 = r.kind == kJitter ? stats[2 * b] : 0.0f, c1 = r.kind == kJitter ? stats[2 * b + 1] : 0.0f;
    const Lin ty = lin_taps(oy, r.ih, OH), tx = lin_taps(ox, r.iw, OW);
    const int ys[2] = {ty.i0, ty.i1}, xs[2] = {tx.i0, tx.i1};
    float vi[4], vm[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const Gather g = locate(r, ys[k >> 1], xs[k & 1]);
        vi[k] = sample(r, g, si, 0.0f, c0);
        if (MK == 0)
            vm[k] = sample(r, g, SrcMaskU8{static_cast<const uint8_t*>(mask) + o}, 0.0f, c1);
        else
            vm[k] = sample(r, g, SrcF32{static_cast<const float*>(mask) + o}, 0.0f, c1);
    }
    const size_t at = ((size_t)b * OH + oy) * OW + ox;
    Elem<T>::st(img_out + at, (vi[0] * tx.l0 + vi[1] * tx.l1) * ty.l0 + (vi[2] * tx.l0 + vi[3] * tx.l1) * ty.l1);
    mask_out[at] = (vm[0] * tx.l0 + vm[1] * tx.l1) * ty.l0 + (vm[2] * tx.l0 + vm[3] * tx.l1) * ty.l1;
}

// ---- recognition -------------------------------------------------------------------------------------------------------------
// offs[b] = {source element offset, intermediate offset in ws, horizontal-pass offset in ws}
template <int KIND>
__global__ __launch_bounds__(256) void k_aug_line_stats(const void* __restrict__ crops, const uint8_t* __restrict__ masks,
                                                        const long long* __restrict__ offs, const int* __restrict__ params, double* __restrict__ part) {
    const int b = blockIdx.z;
    const Rec r = load_rec(params + (size_t)b * kAugRec);
    if (r.kind != kJitter) return;
    const long long o = offs[3 * b];
    const uint8_t* m = masks ? masks + o : nullptr;
    double* out = part + (size_t)b * kStatChunks + blockIdx.x;
    if (KIND == 0)
        stats_chunk(r, SrcMasked<SrcU8>{{static_cast<const uint8_t*>(crops) + o}, m}, out);
    else
        stats_chunk(r, SrcMasked<SrcF32>{{static_cast<const float*>(crops) + o}, m}, out);
}

// background mask + augmentation (+ clamp(-0.5, 0.5)) -> packed fp32 intermediate (ih, iw) per sample; block 64 x 4
template <int KIND>
__global__ __launch_bounds__(256) void k_aug_line_warp(const void* __restrict__ crops, const uint8_t* __restrict__ masks,
                                                       const long long* __restrict__ offs, const int* __restrict__ params,
                                                       const float* __restrict__ stats, float* __restrict__ inter, int clamp) {
    const int b = blockIdx.z;
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    const Rec r = load_rec(params + (size_t)b * kAugRec);
    if (x >= r.iw || y >= r.ih) return;
    const long long o = offs[3 * b];
    const uint8_t* m = masks ? masks + o : nullptr;
    const float cofs = r.kind == kJitter ? stats[b] : 0.0f;
    const Gather g = locate(r, y, x);
    float v = KIND == 0 ? sample(r, g, SrcMasked<SrcU8>{{static_cast<const uint8_t*>(crops) + o}, m}, -0.5f, cofs)
                        : sample(r, g, SrcMasked<SrcF32>{{static_cast<const float*>(crops) + o}, m}, -0.5f, cofs);
    if (clamp) v = fminf(fmaxf(v, -0.5f), 0.5f);
    inter[offs[3 * b + 1] + (long long)y * r.iw + x] = v;
}

// k_resize_aa_h / k_resize_aa_v over variable shapes: intermediate (ih, iw) -> (ih, ow) -> (OH, ow), the vertical pass writing the
// (B, 1, OH, Wpad) collate layout with 0.0 right of ow.  Same weight rule and accumulation as the fixed-shape kernels, so the same bits.
__global__ __launch_bounds__(256) void k_aug_line_h(const long long* __restrict__ offs, const int* __restrict__ params, const float* __restrict__ inter,
                                                    float* __restrict__ hpass) {
    const int b = blockIdx.z, y = blockIdx.y, ox = blockIdx.x * 256 + threadIdx.x;
    const Rec r = load_rec(params + (size_t)b * kAugRec);
    if (ox >= r.ow || y >= r.ih) return;
    const AaSpan s = aa_span(ox, r.iw, (float)r.iw / (float)r.ow);
    const float* src = inter + offs[3 * b + 1] + (long long)y * r.iw + s.lo;
    float acc = 0.0f;
    for (int j = 0; j < s.cnt; ++j) acc += aa_w(s, j) * src[j];
    hpass[offs[3 * b + 2] + (long long)y * r.ow + ox] = acc;
}

template <typename T>
__global__ __launch_bounds__(256) void k_aug_line_v(const long long* __restrict__ offs, const int* __restrict__ params, const float* __restrict__ hpass,
                                                    T* __restrict__ out, int OH, int Wpad) {
    const int b = blockIdx.z, oy = blockIdx.y;
    const int x0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (x0 >= Wpad) return;
    const Rec r = load_rec(params + (size_t)b * kAugRec);
    const AaSpan s = aa_span(oy, r.ih, (float)r.ih / (float)OH);
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int ox = x0 + i;
        float acc = 0.0f;  // pad value 0.0 = mid grey (train_rec.py:295)
        if (ox < r.ow) {
            const float* src = hpass + offs[3 * b + 2] + (long long)s.lo * r.ow + ox;
            for (int j = 0; j < s.cnt; ++j) acc += aa_w(s, j) * src[(long long)j * r.ow];
        }
        v[i] = acc;
    }
    store4(out + ((size_t)b * OH + oy) * Wpad + x0, v[0], v[1], v[2], v[3]);
}


// ws = [B][planes][kStatChunks] fp64 partials, then [B][planes] fp32 contrast terms (rounded up to 4 floats)
long stats_ws_floats(int B, int planes) { return (long)B * planes * kStatChunks * 2 + ((long)B * planes + 3) / 4 * 4; }

}  // namespace

extern "C" {

long ocrs_augment_det_ws_floats(int B) { return B > 0 ? stats_ws_floats(B, 2) : 0; }

int ocrs_augment_det(const void* img_u8, const void* mask, const long long* offs, const int* params, float* ws, void* img_out, float* mask_out,
                     int B, int max_h, int max_w, int OH, int OW, int mask_kind, int dtype, hipStream_t st) {
    OCRS_CHECK_ARG(B >= 0 && B <= 65535 && (mask_kind == 0 || mask_kind == 1) && (dtype == 0 || dtype == 1));
    if (B == 0) return OCRS_OK;
    OCRS_CHECK_ARG(img_u8 && mask && offs && params && ws && img_out && mask_out);
    OCRS_CHECK_ARG(max_h > 0 && max_w > 0 && max_h <= 65535 && max_w <= 65535 && (long long)max_h * max_w < (1LL << 31));
    OCRS_CHECK_ARG(OH > 0 && OW > 0 && OH <= 65535 && OW <= 65535 && (long long)OH * OW < (1LL << 31));
    OCRS_CHECK_ARG(aligned16(params) && aligned16(ws) && aligned16(img_out) && aligned16(mask_out) && (mask_kind == 0 || aligned16(mask)));
    const dim3 sgrid(kStatChunks, 2, B), grid((OW + 63) / 64, (OH + 3) / 4, B), block(64, 4);
    const uint8_t* img = static_cast<const uint8_t*>(img_u8);
    double* part = reinterpret_cast<double*>(ws);
    float* stats = ws + (long)B * 2 * kStatChunks * 2;
    if (mask_kind == 0)
        hipLaunchKernelGGL(k_aug_det_stats<0>, sgrid, dim3(256), 0, st, img, mask, offs, params, part);
    else
        hipLaunchKernelGGL(k_aug_det_stats<1>, sgrid, dim3(256), 0, st, img, mask, offs, params, part);
    hipLaunchKernelGGL(k_aug_stats_fin, dim3((2 * B + 255) / 256), dim3(256), 0, st, params, (const double*)part, stats, B, 2);
#define OCRS_AUG_DET(T_, MK_) \
    hipLaunchKernelGGL((k_aug_det<T_, MK_>), grid, block, 0, st, img, mask, offs, params, (const float*)stats, static_cast<T_*>(img_out), mask_out, OH, OW)
    if (dtype == 0 && mask_kind == 0) OCRS_AUG_DET(float, 0);
    else if (dtype == 0) OCRS_AUG_DET(float, 1);
    else if (mask_kind == 0) OCRS_AUG_DET(bf16, 0);
    else OCRS_AUG_DET(bf16, 1);
#undef OCRS_AUG_DET
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

long ocrs_augment_lines_ws_floats(int B, long inter_floats, long hpass_floats) {
    if (B < 0 || inter_floats < 0 || hpass_floats < 0) return 0;
    return stats_ws_floats(B, 1) + (inter_floats + 3) / 4 * 4 + hpass_floats;
}

int ocrs_augment_lines(const void* crops, const void* masks, const long long* offs, const int* params, float* ws, long inter_floats, void* out, int B,
                       int max_ih, int max_iw, int OH, int Wpad, int kind, int clamp, int dtype, hipStream_t st) {
    OCRS_CHECK_ARG(B >= 0 && B <= 65535 && (kind == 0 || kind == 1) && (dtype == 0 || dtype == 1) && inter_floats >= 0);
    if (B == 0) return OCRS_OK;
    OCRS_CHECK_ARG(crops && offs && params && ws && out && (kind == 0 || aligned16(crops)));
    OCRS_CHECK_ARG(max_ih > 0 && max_iw > 0 && max_ih <= 65535 && max_iw <= 65535 && (long long)max_ih * max_iw < (1LL << 31));
    OCRS_CHECK_ARG(OH > 0 && OH <= 65535 && Wpad > 0 && Wpad % 4 == 0 && Wpad <= 65535);
    OCRS_CHECK_ARG(aligned16(params) && aligned16(ws) && aligned16(out));
    double* part = reinterpret_cast<double*>(ws);
    float* stats = ws + (long)B * kStatChunks * 2;
    float* inter = ws + stats_ws_floats(B, 1);
    float* hpass = inter + (inter_floats + 3) / 4 * 4;
    const uint8_t* m = static_cast<const uint8_t*>(masks);
    const dim3 sgrid(kStatChunks, 1, B), wgrid((max_iw + 63) / 64, (max_ih + 3) / 4, B);
    if (kind == 0)
        hipLaunchKernelGGL(k_aug_line_stats<0>, sgrid, dim3(256), 0, st, crops, m, offs, params, part);
    else
        hipLaunchKernelGGL(k_aug_line_stats<1>, sgrid, dim3(256), 0, st, crops, m, offs, params, part);
    hipLaunchKernelGGL(k_aug_stats_fin, dim3((B + 255) / 256), dim3(256), 0, st, params, (const double*)part, stats, B, 1);
    if (kind == 0)
        hipLaunchKernelGGL(k_aug_line_warp<0>, wgrid, dim3(64, 4), 0, st, crops, m, offs, params, (const float*)stats, inter, clamp);
    else
        hipLaunchKernelGGL(k_aug_line_warp<1>, wgrid, dim3(64, 4), 0, st, crops, m, offs, params, (const float*)stats, inter, clamp);
    hipLaunchKernelGGL(k_aug_line_h, dim3((Wpad + 255) / 256, max_ih, B), dim3(256), 0, st, offs, params, (const float*)inter, hpass);
    if (dtype == 0)
        hipLaunchKernelGGL(k_aug_line_v<float>, dim3((Wpad / 4 + 255) / 256, OH, B), dim3(256), 0, st, offs, params, (const float*)hpass,
                           static_cast<float*>(out), OH, Wpad);
    else
        hipLaunchKernelGGL(k_aug_line_v<bf16>, dim3((Wpad / 4 + 255) / 256, OH, B), dim3(256), 0, st, offs, params, (const float*)hpass,
                           static_cast<bf16*>(out), OH, Wpad);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

}  // extern "C"
