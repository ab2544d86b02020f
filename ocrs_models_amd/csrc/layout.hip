// Layout model (ocrs_models/models.py:271-406, train_layout.py:15-171): everything between the Linear layers of the transformer encoder.
//   embedding          boxes -> sinusoidal encodings, computed per element (no table, no host synchronisation)
//   attention          one workgroup per (word, head): softmax(Q K^T / 8) V on v_mfma_f32_16x16x4_f32, probabilities stay in registers;
//                      the backward recomputes them and writes dQ | dK | dV into the in-projection's output gradient
//   residual + dropout + LayerNorm, forward and backward, one wave per 256-float row
//   ReLU + dropout on the feed-forward hidden, weighted BCE-with-logits + accuracy counts, fixed-order column sums
// All storage fp32.  Dropout masks are Philox-4x32-10 words keyed by (seed, site) with the element index as the counter: the backward
// regenerates them, nothing is stored.  Every reduction is a fixed-order sum (bit-reproducible); reductions end in plain vector stores.
#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------------------------------
// counter-based dropout
struct DropKey {
    unsigned k0, k1, site, thr;  // keep an element iff its 32-bit word >= thr (thr = p * 2^32)
    float scale;                 // 1 / (1 - p)
    int on;
};

static DropKey make_key(float p, long seed, int site) {
    DropKey k;
    k.on = p > 0.f;
    k.k0 = (unsigned)((unsigned long long)seed & 0xffffffffull);
    k.k1 = (unsigned)((unsigned long long)seed >> 32);
    k.site = (unsigned)site;
    k.thr = k.on ? (unsigned)((double)p * 4294967296.0) : 0u;
    k.scale = k.on ? 1.f / (1.f - p) : 1.f;
    return k;
}

// Philox-4x32-10 (Salmon et al., SC'11): counter = (group lo, group hi, site, 0), key = seed; one call yields the words of 4 consecutive elements
__device__ __forceinline__ uint4 philox4(const DropKey& k, unsigned long long group) {
    unsigned c0 = (unsigned)group, c1 = (unsigned)(group >> 32), c2 = k.site, c3 = 0u;
    unsigned k0 = k.k0, k1 = k.k1;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return make_uint4(c0, c1, c2, c3);
}
// element idx: word (idx & 3) of group idx >> 2
__device__ __forceinline__ bool keep1(const DropKey& k, unsigned long long idx) {
    const uint4 w = philox4(k, idx >> 2);
    const unsigned s = (unsigned)idx & 3u;
    const unsigned v = s == 0 ? w.x : (s == 1 ? w.y : (s == 2 ? w.z : w.w));
    return v >= k.thr;
}

__global__ __launch_bounds__(256) void k_lay_mask(unsigned char* __restrict__ mask, long n, DropKey dk) {
    for (long g = (long)blockIdx.x * 256 + threadIdx.x; g * 4 < n; g += (long)gridDim.x * 256) {
        const uint4 w = philox4(dk, (unsigned long long)g);
        const unsigned v[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (g * 4 + i < n) mask[g * 4 + i] = v[i] >= dk.thr ? 1 : 0;
    }
}

__device__ __forceinline__ float4 drop4(const DropKey& dk, unsigned long long group, float4 v) {
    const uint4 w = philox4(dk, group);
    v.x = w.x >= dk.thr ? v.x * dk.scale : 0.f;
    v.y = w.y >= dk.thr ? v.y * dk.scale : 0.f;
    v.z = w.z >= dk.thr ? v.z * dk.scale : 0.f;
    v.w = w.w >= dk.thr ? v.w * dk.scale : 0.f;
    return v;
}

static inline int lay_grid(long items, int per_cu = 8) {
    long g = (items + 255) / 256;
    const long cap = (long)kNumCU * per_cu;
    return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

// ---------------------------------------------------------------------------------------------------------------------
// SinPositionalEncoding(256) (models.py:271-337): out[row][c * 64 + j] = sin(p * r_j), out[row][c * 64 + 32 + j] = cos(p * r_j),
// p = round-half-even(box[row][c]), the angle rounded once to fp32 -- the values the reference gathers from its table.
__global__ __launch_bounds__(256) void k_lay_embed(const float* __restrict__ boxes, const float* __restrict__ rates, float* __restrict__ out, long rows) {
    const long n = rows * 128;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const long row = i >> 7;
        const int c = (int)(i >> 5) & 3, j = (int)i & 31;
        const float p = (float)(int)rintf(boxes[row * 4 + c]);
        const float ang = __fmul_rn(p, rates[j]);
        out[row * 256 + c * 64 + j] = sinf(ang);
        out[row * 256 + c * 64 + 32 + j] = cosf(ang);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Attention.  qkv [S][W][768] (q | k | v, each 4 heads x 64), sequence stride W * 768 (batch_first=False: the sequence axis is the page axis).
// MFMA 16x16x4 fp32 operand layout: A lane l = A[l & 15][l >> 4], B lane l = B[l >> 4][l & 15], D lane l reg r = D[4 * (l >> 4) + r][l & 15].
// Scores are formed TRANSPOSED (keys x queries): D reg r of key tile t is then exactly the B operand (k index = key 4 * (l >> 4) + r) of the
// P^T-consuming products, so the probabilities never leave the registers.
constexpr int ALD = 68;  // LDS row pitch in floats: 16-byte aligned rows, conflict-free for both fragment read patterns

template <int NT>
__device__ __forceinline__ void lay_stage(float* dst, const float* __restrict__ src, long seq_stride, int S, int tid) {
    for (int i = tid; i < NT * 16 * 16; i += 256) {
        const int s = i >> 4, c = (i & 15) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (s < S) v = *reinterpret_cast<const float4*>(src + (long)s * seq_stride + c);
        *reinterpret_cast<float4*>(dst + s * ALD + c) = v;
    }
}

// T[t][r] = sum_d A[(16 t + li)][d] * B[(bt * 16 + li)][d]: rows of A on the D rows, rows of B on the D columns
template <int NT>
__device__ __forceinline__ void lay_outer(const float* As, const float* Bs, int bt, int lane, f32x4 (&acc)[NT]) {
    const int g = lane >> 4, li = lane & 15;
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int ks = 0; ks < 16; ++ks) {
        const float b = Bs[(bt * 16 + li) * ALD + ks * 4 + g];
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(As[(t * 16 + li) * ALD + ks * 4 + g], b, acc[t], 0, 0, 0);
    }
}

// O^T[d][col] = sum_{t, r} Xs[16 t + 4 g + r][16 dc + li] * P[t][r]  ->  lane holds O[col = li][d = 16 dc + 4 g + 0..3]
template <int NT>
__device__ __forceinline__ f32x4 lay_inner(const float* Xs, const f32x4 (&p)[NT], int dc, int lane) {
    const int g = lane >> 4, li = lane & 15;
    f32x4 o = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) o = __builtin_amdgcn_mfma_f32_16x16x4f32(Xs[(t * 16 + 4 * g + r) * ALD + dc * 16 + li], p[t][r], o, 0, 0, 0);
    return o;
}

__device__ __forceinline__ float xg_max(float v) {  // over the four 16-lane groups
    v = fmaxf(v, __shfl_xor(v, 16));
    return fmaxf(v, __shfl_xor(v, 32));
}
__device__ __forceinline__ float xg_sum(float v) {
    v += __shfl_xor(v, 16);
    return v + __shfl_xor(v, 32);
}

// softmax over the keys of transposed scores acc[t][r] (key 16 t + 4 g + r, query on the lane): returns row max and 1 / sum
template <int NT>
__device__ __forceinline__ void lay_softmax_t(f32x4 (&acc)[NT], int S, int lane, float& mx, float& inv) {
    const int g = lane >> 4;
    mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float s = t * 16 + 4 * g + r < S ? acc[t][r] * 0.125f : -INFINITY;
            acc[t][r] = s;
            mx = fmaxf(mx, s);
        }
    mx = xg_max(mx);
    float sum = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float e = expf(acc[t][r] - mx);  // (keys >= S: exp(-inf) = 0)
            acc[t][r] = e;
            sum += e;
        }
    sum = xg_sum(sum);
    inv = 1.f / sum;
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] *= inv;
}

template <int NT>
__global__ __launch_bounds__(256) void k_lay_attn_fwd(const float* __restrict__ qkv, float* __restrict__ out, int S, int W, DropKey dk) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    constexpr int SP = NT * 16;
    float *Qs = sm, *Ks = Qs + SP * ALD, *Vs = Ks + SP * ALD;
    const int w = blockIdx.x, h = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
    const float* base = qkv + (long)w * 768 + h * 64;
    const long ss = (long)W * 768;
    lay_stage<NT>(Qs, base, ss, S, tid);
    lay_stage<NT>(Ks, base + 256, ss, S, tid);
    lay_stage<NT>(Vs, base + 512, ss, S, tid);
    __syncthreads();
    for (int qt = wave; qt < NT; qt += 4) {
        f32x4 p[NT];
        lay_outer<NT>(Ks, Qs, qt, lane, p);  // p[t][r]: key 16 t + 4 g + r, query qt * 16 + li
        float mx, inv;
        lay_softmax_t<NT>(p, S, lane, mx, inv);
        const int q = qt * 16 + li;
        if (dk.on) {
            const unsigned long long row = ((unsigned long long)(w * 4 + h) * S + q) * S;
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = t * 16 + 4 * g + r;
                    if (q < S && key < S) p[t][r] = keep1(dk, row + key) ? p[t][r] * dk.scale : 0.f;
                }
        }
#pragma unroll
        for (int dc = 0; dc < 4; ++dc) {
            const f32x4 o = lay_inner<NT>(Vs, p, dc, lane);
            if (q < S) *reinterpret_cast<float4*>(out + ((long)q * W + w) * 256 + h * 64 + dc * 16 + 4 * g) = make_float4(o[0], o[1], o[2], o[3]);
        }
    }
}

// Backward.  Phase A (a wave per query tile): transposed scores -> probabilities, row statistics to LDS, dS^T -> dQ.
// Phase B (a wave per key tile): scores in the other orientation (queries x keys) from the saved row statistics -> dS -> dK, dV.
template <int NT>
__global__ __launch_bounds__(256) void k_lay_attn_bwd(const float* __restrict__ qkv, const float* __restrict__ dout, float* __restrict__ dqkv, int S, int W,
                                                      DropKey dk) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    constexpr int SP = NT * 16;
    float *Qs = sm, *Ks = Qs + SP * ALD, *Vs = Ks + SP * ALD, *Gs = Vs + SP * ALD;
    float *mrow = Gs + SP * ALD, *irow = mrow + SP, *drow = irow + SP;
    const int w = blockIdx.x, h = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, li = lane & 15;
    const float* base = qkv + (long)w * 768 + h * 64;
    const long ss = (long)W * 768;
    lay_stage<NT>(Qs, base, ss, S, tid);
    lay_stage<NT>(Ks, base + 256, ss, S, tid);
    lay_stage<NT>(Vs, base + 512, ss, S, tid);
    lay_stage<NT>(Gs, dout + (long)w * 256 + h * 64, (long)W * 256, S, tid);
    __syncthreads();
    const unsigned long long head = (unsigned long long)(w * 4 + h) * S;
    for (int qt = wave; qt < NT; qt += 4) {
        f32x4 p[NT], dp[NT];
        lay_outer<NT>(Ks, Qs, qt, lane, p);
        float mx, inv;
        lay_softmax_t<NT>(p, S, lane, mx, inv);
        lay_outer<NT>(Vs, Gs, qt, lane, dp);  // dPd^T[key][query] = V[key] . dO[query]
        const int q = qt * 16 + li;
        float delta = 0.f;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = t * 16 + 4 * g + r;
                if (dk.on && q < S && key < S) dp[t][r] = keep1(dk, (head + q) * S + key) ? dp[t][r] * dk.scale : 0.f;  // dP = mask / (1 - p) * dPd
                delta += dp[t][r] * p[t][r];
            }
        delta = xg_sum(delta);
        if (g == 0) {
            mrow[q] = mx;
            irow[q] = inv;
            drow[q] = delta;
        }
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) p[t][r] = p[t][r] * (dp[t][r] - delta) * 0.125f;  // dS^T (scaled for dQ)
#pragma unroll
        for (int dc = 0; dc < 4; ++dc) {
            const f32x4 o = lay_inner<NT>(Ks, p, dc, lane);
            if (q < S) *reinterpret_cast<float4*>(dqkv + ((long)q * W + w) * 768 + h * 64 + dc * 16 + 4 * g) = make_float4(o[0], o[1], o[2], o[3]);
        }
    }
    __syncthreads();
    for (int kt = wave; kt < NT; kt += 4) {
        f32x4 p[NT], dp[NT];
        lay_outer<NT>(Qs, Ks, kt, lane, p);   // p[t][r]: query 16 t + 4 g + r, key kt * 16 + li
        lay_outer<NT>(Gs, Vs, kt, lane, dp);  // dPd[query][key]
        const int key = kt * 16 + li;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int q = t * 16 + 4 * g + r;
                const bool in = q < S && key < S;
                float pv = in ? expf(p[t][r] * 0.125f - mrow[q]) * irow[q] : 0.f;
                float dpv = dp[t][r];
                float pd = pv;
                if (dk.on && in) {
                    const bool kp = keep1(dk, (head + q) * S + key);
                    dpv = kp ? dpv * dk.scale : 0.f;
                    pd = kp ? pv * dk.scale : 0.f;
                }
                dp[t][r] = in ? pv * (dpv - drow[q]) * 0.125f : 0.f;  // dS
                p[t][r] = pd;                                         // dropped probabilities (dV)
            }
#pragma unroll
        for (int dc = 0; dc < 4; ++dc) {
            const f32x4 ok = lay_inner<NT>(Qs, dp, dc, lane);
            const f32x4 ov = lay_inner<NT>(Gs, p, dc, lane);
            if (key < S) {
                float* o = dqkv + ((long)key * W + w) * 768 + h * 64 + dc * 16 + 4 * g;
                *reinterpret_cast<float4*>(o + 256) = make_float4(ok[0], ok[1], ok[2], ok[3]);
                *reinterpret_cast<float4*>(o + 512) = make_float4(ov[0], ov[1], ov[2], ov[3]);
            }
        }
    }
}

static size_t attn_fwd_lds(int nt) { return (size_t)3 * nt * 16 * ALD * sizeof(float); }
static size_t attn_bwd_lds(int nt) { return ((size_t)4 * nt * 16 * ALD + 3 * nt * 16) * sizeof(float); }


// ---------------------------------------------------------------------------------------------------------------------
// y = LayerNorm(x + dropout(a)) over rows of 256 floats, one wave per row (lane = 4 columns); stat [rows][2] = mean | rstd.
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(256) void k_lay_ln_fwd(const float* __restrict__ x, const float* __restrict__ a, const float* __restrict__ gamma,
                                                    const float* __restrict__ beta, float* __restrict__ y, float* __restrict__ stat, long rows, float eps,
                                                    DropKey dk) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float4 gm = reinterpret_cast<const float4*>(gamma)[lane], bt = reinterpret_cast<const float4*>(beta)[lane];
    for (long row = (long)blockIdx.x * 4 + wave; row < rows; row += (long)gridDim.x * 4) {
        const float4 xv = reinterpret_cast<const float4*>(x + row * 256)[lane];
        float4 av = reinterpret_cast<const float4*>(a + row * 256)[lane];
        if (dk.on) av = drop4(dk, (unsigned long long)row * 64 + lane, av);
        const float s0 = xv.x + av.x, s1 = xv.y + av.y, s2 = xv.z + av.z, s3 = xv.w + av.w;
        const float mean = wave_sum((s0 + s1) + (s2 + s3)) * (1.f / 256.f);
        const float d0 = s0 - mean, d1 = s1 - mean, d2 = s2 - mean, d3 = s3 - mean;
        const float var = wave_sum((d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3)) * (1.f / 256.f);
        const float rstd = 1.f / sqrtf(var + eps);
        reinterpret_cast<float4*>(y + row * 256)[lane] =
            make_float4(d0 * rstd * gm.x + bt.x, d1 * rstd * gm.y + bt.y, d2 * rstd * gm.z + bt.z, d3 * rstd * gm.w + bt.w);
        if (stat && lane == 0) {
            stat[row * 2] = mean;
            stat[row * 2 + 1] = rstd;
        }
    }
}

// Backward of the same: dy = dy1 (+ dy2), s = x + dropout(a) recomputed.  ds [rows][256] = dL/ds (the residual branch's gradient),
// da (nullable; written when dropout is on) = mask / (1 - p) * ds.  part [gridDim.x][512] = this workgroup's dgamma | dbeta sums.
__global__ __launch_bounds__(256) void k_lay_ln_bwd(const float* __restrict__ dy1, const float* __restrict__ dy2, const float* __restrict__ x,
                                                    const float* __restrict__ a, const float* __restrict__ stat, const float* __restrict__ gamma,
                                                    float* __restrict__ ds, float* __restrict__ da, float* __restrict__ part, long rows, DropKey dk) {
    __shared__ float red[4][512];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float4 gm = reinterpret_cast<const float4*>(gamma)[lane];
    float dg[4] = {0.f, 0.f, 0.f, 0.f}, db[4] = {0.f, 0.f, 0.f, 0.f};
    for (long row = (long)blockIdx.x * 4 + wave; row < rows; row += (long)gridDim.x * 4) {
        const float4 xv = reinterpret_cast<const float4*>(x + row * 256)[lane];
        float4 av = reinterpret_cast<const float4*>(a + row * 256)[lane];
        float4 gy = reinterpret_cast<const float4*>(dy1 + row * 256)[lane];
        if (dy2) {
            const float4 g2 = reinterpret_cast<const float4*>(dy2 + row * 256)[lane];
            gy.x += g2.x, gy.y += g2.y, gy.z += g2.z, gy.w += g2.w;
        }
        uint4 wd = make_uint4(~0u, ~0u, ~0u, ~0u);
        if (dk.on) {
            wd = philox4(dk, (unsigned long long)row * 64 + lane);
            av.x = wd.x >= dk.thr ? av.x * dk.scale : 0.f;
            av.y = wd.y >= dk.thr ? av.y * dk.scale : 0.f;
            av.z = wd.z >= dk.thr ? av.z * dk.scale : 0.f;
            av.w = wd.w >= dk.thr ? av.w * dk.scale : 0.f;
        }
        const float mean = stat[row * 2], rstd = stat[row * 2 + 1];
        const float h0 = (xv.x + av.x - mean) * rstd, h1 = (xv.y + av.y - mean) * rstd, h2 = (xv.z + av.z - mean) * rstd, h3 = (xv.w + av.w - mean) * rstd;
        const float g0 = gy.x * gm.x, g1 = gy.y * gm.y, g2 = gy.z * gm.z, g3 = gy.w * gm.w;
        const float m1 = wave_sum((g0 + g1) + (g2 + g3)) * (1.f / 256.f);
        const float m2 = wave_sum((g0 * h0 + g1 * h1) + (g2 * h2 + g3 * h3)) * (1.f / 256.f);
        const float4 o = make_float4(rstd * (g0 - m1 - h0 * m2), rstd * (g1 - m1 - h1 * m2), rstd * (g2 - m1 - h2 * m2), rstd * (g3 - m1 - h3 * m2));
        reinterpret_cast<float4*>(ds + row * 256)[lane] = o;
        if (dk.on)
            reinterpret_cast<float4*>(da + row * 256)[lane] =
                make_float4(wd.x >= dk.thr ? o.x * dk.scale : 0.f, wd.y >= dk.thr ? o.y * dk.scale : 0.f, wd.z >= dk.thr ? o.z * dk.scale : 0.f,
                            wd.w >= dk.thr ? o.w * dk.scale : 0.f);
        dg[0] += gy.x * h0, dg[1] += gy.y * h1, dg[2] += gy.z * h2, dg[3] += gy.w * h3;
        db[0] += gy.x, db[1] += gy.y, db[2] += gy.z, db[3] += gy.w;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        red[wave][lane * 4 + i] = dg[i];
        red[wave][256 + lane * 4 + i] = db[i];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 512; i += 256) part[(long)blockIdx.x * 512 + i] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
}

// out[c] = sum_b ws[b][c] (c < nout), b in a fixed order: four interleaved chains, then ((0 + 1) + (2 + 3))
__global__ __launch_bounds__(256) void k_lay_colreduce(const float* __restrict__ ws, int nb, int n, float* __restrict__ out0, int n0, float* __restrict__ out1,
                                                       int n1) {
    __shared__ float red[4][64];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), part = threadIdx.x >> 6;
    float s = 0.f;
    if (c < n)
        for (int b = part; b < nb; b += 4) s += ws[(long)b * n + c];
    red[part][threadIdx.x & 63] = s;
    __syncthreads();
    if (part == 0 && c < n) {
        const int l = threadIdx.x & 63;
        const float v = (red[0][l] + red[1][l]) + (red[2][l] + red[3][l]);
        if (c < n0)
            out0[c] = v;
        else if (c - n0 < n1)
            out1[c - n0] = v;
    }
}

// per-workgroup column sums of a [rows][ld] (C % 4 == 0 columns): ws [gridDim.x][C]
__global__ __launch_bounds__(256) void k_lay_colsum(const float* __restrict__ a, int ld, int C, long rows, float* __restrict__ ws) {
    __shared__ float4 red[4][64];
    const int cg = blockIdx.y * 64 + (threadIdx.x & 63), sub = threadIdx.x >> 6;
    const long chunk = (rows + gridDim.x - 1) / gridDim.x;
    const long r0 = (long)blockIdx.x * chunk, r1 = r0 + chunk < rows ? r0 + chunk : rows;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (cg * 4 < C)
        for (long r = r0 + sub; r < r1; r += 4) {
            const float4 v = *reinterpret_cast<const float4*>(a + r * ld + cg * 4);
            s.x += v.x, s.y += v.y, s.z += v.z, s.w += v.w;
        }
    red[sub][threadIdx.x & 63] = s;
    __syncthreads();
    if (sub == 0 && cg * 4 < C) {
        const int l = threadIdx.x & 63;
        const float4 p0 = red[0][l], p1 = red[1][l], p2 = red[2][l], p3 = red[3][l];
        *reinterpret_cast<float4*>(ws + (long)blockIdx.x * C + cg * 4) =
            make_float4((p0.x + p1.x) + (p2.x + p3.x), (p0.y + p1.y) + (p2.y + p3.y), (p0.z + p1.z) + (p2.z + p3.z), (p0.w + p1.w) + (p2.w + p3.w));
    }
}

static inline int colsum_blocks(long rows) {
    long nb = (rows + 63) / 64;
    return (int)(nb < 1 ? 1 : (nb > 256 ? 256 : nb));
}
static inline int ln_bwd_blocks(long rows) {
    long nb = (rows + 31) / 32;  // >= 8 rows per wave before another workgroup is worth its 512 partials
    return (int)(nb < 1 ? 1 : (nb > 512 ? 512 : nb));
}

// ---------------------------------------------------------------------------------------------------------------------
// ReLU + dropout on the feed-forward hidden, in place; the backward needs only the stored value: it is > 0 exactly where the ReLU was open
// and the element kept.
__global__ __launch_bounds__(256) void k_lay_relu_drop(float* __restrict__ h, long n4, int relu, DropKey dk) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        float4 v = reinterpret_cast<float4*>(h)[i];
        if (relu) v = make_float4(fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f));
        if (dk.on) v = drop4(dk, (unsigned long long)i, v);
        reinterpret_cast<float4*>(h)[i] = v;
    }
}
__global__ __launch_bounds__(256) void k_lay_relu_drop_bwd(const float* __restrict__ g, const float* __restrict__ h, float* __restrict__ out, long n4, float scale) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const float4 gv = reinterpret_cast<const float4*>(g)[i], hv = reinterpret_cast<const float4*>(h)[i];
        reinterpret_cast<float4*>(out)[i] =
            make_float4(hv.x > 0.f ? gv.x * scale : 0.f, hv.y > 0.f ? gv.y * scale : 0.f, hv.z > 0.f ? gv.z * scale : 0.f, hv.w > 0.f ? gv.w * scale : 0.f);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// head: compact the padded logits [rows][ld] to [rows][2] (optionally through the sigmoid), and the reverse for the gradient
__global__ __launch_bounds__(256) void k_lay_head_out(const float* __restrict__ logits, int ld, float* __restrict__ out, long rows, int probs) {
    for (long r = (long)blockIdx.x * 256 + threadIdx.x; r < rows; r += (long)gridDim.x * 256) {
        float a = logits[r * ld], b = logits[r * ld + 1];
        if (probs) a = 1.f / (1.f + expf(-a)), b = 1.f / (1.f + expf(-b));
        reinterpret_cast<float2*>(out)[r] = make_float2(a, b);
    }
}
__global__ __launch_bounds__(256) void k_lay_head_grad_in(const float* __restrict__ g, float* __restrict__ dlog, int ld, long rows) {
    const int ld4 = ld / 4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < rows * ld4; i += (long)gridDim.x * 256) {
        const long r = i / ld4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i % ld4 == 0) {
            const float2 t = reinterpret_cast<const float2*>(g)[r];
            v.x = t.x, v.y = t.y;
        }
        reinterpret_cast<float4*>(dlog)[i] = v;
    }
}

// BCEWithLogitsLoss(pos_weight) mean (train_layout.py:94-97), its gradient and the counts of LayoutAccuracyStats.update (train_layout.py:46-63)
struct LossPart {
    double loss;
    long long cnt[6];
    long long pad;
};
constexpr int LOSS_MAXB = 256;
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__global__ __launch_bounds__(256) void k_lay_loss(const float* __restrict__ pred, const float* __restrict__ target, float pw, int pred_is_prob,
                                                  float* __restrict__ loss_out, float* __restrict__ dlogits, long long* __restrict__ counts,
                                                  LossPart* __restrict__ parts, unsigned* __restrict__ counter, long rows) {
    __shared__ double s_loss[4];
    __shared__ int s_cnt[4][6];
    __shared__ bool s_last;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float gscale = 1.f / (float)(rows * 2);
    double loss = 0.0;
    int cnt[6] = {0, 0, 0, 0, 0, 0};
    for (long r = (long)blockIdx.x * 256 + threadIdx.x; r < rows; r += (long)gridDim.x * 256) {
        const float2 xv = reinterpret_cast<const float2*>(pred)[r], tv = reinterpret_cast<const float2*>(target)[r];
        const float xs[2] = {xv.x, xv.y}, ts[2] = {tv.x, tv.y};
        float gr[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const float x = xs[c], t = ts[c];
            const float lw = 1.f + (pw - 1.f) * t;
            const float e = expf(-fabsf(x));
            loss += (double)((1.f - t) * x + lw * (log1pf(e) + fmaxf(-x, 0.f)));
            const float sig = x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
            gr[c] = ((1.f - t) - lw * (1.f - sig)) * gscale;
            // the reference thresholds clamp(sigmoid(x), 0, 1) in fp32 (train_layout.py:131) or, in test(), the probabilities it was given
            const bool pp = pred_is_prob ? x >= 0.5f : 1.f / (1.f + expf(-x)) >= 0.5f;
            const bool tp = t != 0.f;
            cnt[3 * c] += pp && tp;
            cnt[3 * c + 1] += pp;
            cnt[3 * c + 2] += tp;
        }
        if (dlogits) reinterpret_cast<float2*>(dlogits)[r] = make_float2(gr[0], gr[1]);
    }
    loss = wave_sum_d(loss);
#pragma unroll
    for (int i = 0; i < 6; ++i) cnt[i] = wave_sum_i(cnt[i]);
    if (lane == 0) {
        s_loss[wave] = loss;
        for (int i = 0; i < 6; ++i) s_cnt[wave][i] = cnt[i];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        LossPart p;
        p.loss = (s_loss[0] + s_loss[1]) + (s_loss[2] + s_loss[3]);
        for (int i = 0; i < 6; ++i) p.cnt[i] = (long long)s_cnt[0][i] + s_cnt[1][i] + s_cnt[2][i] + s_cnt[3][i];
        p.pad = 0;
        parts[blockIdx.x] = p;
        __threadfence();
        s_last = atomicAdd(counter, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!s_last || wave != 0) return;
    __threadfence();
    const volatile LossPart* vp = parts;
    double tl = 0.0;
    long long tc[6] = {0, 0, 0, 0, 0, 0};
    for (int b = lane; b < (int)gridDim.x; b += 64) {  // (fixed order for a given grid: the grid depends on `rows` only)
        tl += vp[b].loss;
        for (int i = 0; i < 6; ++i) tc[i] += vp[b].cnt[i];
    }
    tl = wave_sum_d(tl);
    for (int i = 0; i < 6; ++i) tc[i] = (long long)wave_sum_d((double)tc[i]);  // (counts < 2^53: exact)
    if (lane == 0) {
        loss_out[0] = (float)(tl / (double)(rows * 2));
        if (counts)
            for (int i = 0; i < 6; ++i) counts[i] = tc[i];
        *counter = 0u;
    }
}

// precision_recall (train_layout.py:24-35: int64 counts divided as fp32, 0 / 0 = NaN) of both classes, added to the running sums
// sums [5] fp64 = line-start precision | recall | line-end precision | recall | number of updates
__global__ void k_lay_stats_update(const long long* __restrict__ counts, double* __restrict__ sums) {
    if (threadIdx.x == 0) {
        for (int c = 0; c < 2; ++c) {
            const float tp = (float)counts[3 * c], pp = (float)counts[3 * c + 1], tg = (float)counts[3 * c + 2];
            sums[2 * c] += (double)(tp / pp);
            sums[2 * c + 1] += (double)(tp / tg);
        }
        sums[4] += 1.0;
    }
}

}  // namespace

extern "C" {

int ocrs_layout_embed(const float* boxes, const float* rates, float* out, long rows, hipStream_t st) {
    OCRS_CHECK_ARG(boxes && rates && out && rows > 0);
    hipLaunchKernelGGL(k_lay_embed, dim3(lay_grid(rows * 128)), dim3(256), 0, st, boxes, rates, out, rows);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

long ocrs_layout_attn_supported(int S) { return S >= 1 && S <= 128 ? 1 : 0; }

#define LAY_ATTN_DISPATCH(NT_, CALL) \
    switch (NT_) {                   \
        case 1: CALL(1); break;      \
        case 2: CALL(2); break;      \
        case 3: CALL(3); break;      \
        case 4: CALL(4); break;      \
        case 5: CALL(5); break;      \
        case 6: CALL(6); break;      \
        case 7: CALL(7); break;      \
        default: CALL(8); break;     \
    }

int ocrs_layout_attn_fwd(const float* qkv, float* out, int S, int W, float p, long seed, int site, hipStream_t st) {
    OCRS_CHECK_ARG(qkv && out && ocrs_layout_attn_supported(S) && W >= 1 && W <= 65535 && p >= 0.f && p < 1.f);
    OCRS_CHECK_ARG(((reinterpret_cast<uintptr_t>(qkv) | reinterpret_cast<uintptr_t>(out)) & 15) == 0);
    const DropKey dk = make_key(p, seed, site);
    const int nt = (S + 15) / 16;
#define CALL(N_)                                                                   \
    if (int rc = dyn_lds<&k_lay_attn_fwd<N_>>((int)attn_fwd_lds(N_))) return rc; \
    hipLaunchKernelGGL(k_lay_attn_fwd<N_>, dim3(W, 4), dim3(256), attn_fwd_lds(N_), st, qkv, out, S, W, dk)
    LAY_ATTN_DISPATCH(nt, CALL)
#undef CALL
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

int ocrs_layout_attn_bwd(const float* qkv, const float* dout, float* dqkv, int S, int W, float p, long seed, int site, hipStream_t st) {
    OCRS_CHECK_ARG(qkv && dout && dqkv && ocrs_layout_attn_supported(S) && W >= 1 && W <= 65535 && p >= 0.f && p < 1.f);
    OCRS_CHECK_ARG(((reinterpret_cast<uintptr_t>(qkv) | reinterpret_cast<uintptr_t>(dout) | reinterpret_cast<uintptr_t>(dqkv)) & 15) == 0);
    const DropKey dk = make_key(p, seed, site);
    const int nt = (S + 15) / 16;
#define CALL(N_)                                                                   \
    if (int rc = dyn_lds<&k_lay_attn_bwd<N_>>((int)attn_bwd_lds(N_))) return rc; \
    hipLaunchKernelGGL(k_lay_attn_bwd<N_>, dim3(W, 4), dim3(256), attn_bwd_lds(N_), st, qkv, dout, dqkv, S, W, dk)
    LAY_ATTN_DISPATCH(nt, CALL)
#undef CALL
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

int ocrs_layout_ln_fwd(const float* x, const float* a, const float* gamma, const float* beta, float* y, float* stat, long rows, float eps, float p, long seed,
                       int site, hipStream_t st) {
    OCRS_CHECK_ARG(x && a && gamma && beta && y && rows > 0 && p >= 0.f && p < 1.f);
    OCRS_CHECK_ARG(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(gamma) |
                     reinterpret_cast<uintptr_t>(beta)) & 15) == 0);
    hipLaunchKernelGGL(k_lay_ln_fwd, dim3(lay_grid(rows * 64)), dim3(256), 0, st, x, a, gamma, beta, y, stat, rows, eps, make_key(p, seed, site));
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

long ocrs_layout_ln_bwd_ws_floats(long rows) { return (long)ln_bwd_blocks(rows) * 512; }

int ocrs_layout_ln_bwd(const float* dy1, const float* dy2, const float* x, const float* a, const float* stat, const float* gamma, float* ds, float* da,
                       float* dgamma, float* dbeta, float* ws, long rows, float p, long seed, int site, hipStream_t st) {
    OCRS_CHECK_ARG(dy1 && x && a && stat && gamma && ds && dgamma && dbeta && ws && rows > 0 && p >= 0.f && p < 1.f && (p == 0.f || da));
    OCRS_CHECK_ARG(((reinterpret_cast<uintptr_t>(dy1) | reinterpret_cast<uintptr_t>(dy2) | reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(a) |
                     reinterpret_cast<uintptr_t>(gamma) | reinterpret_cast<uintptr_t>(ds) | reinterpret_cast<uintptr_t>(da)) & 15) == 0);
    const int nb = ln_bwd_blocks(rows);
    hipLaunchKernelGGL(k_lay_ln_bwd, dim3(nb), dim3(256), 0, st, dy1, dy2, x, a, stat, gamma, ds, da, ws, rows, make_key(p, seed, site));
    hipLaunchKernelGGL(k_lay_colreduce, dim3(8), dim3(256), 0, st, (const float*)ws, nb, 512, dgamma, 256, dbeta, 256);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

int ocrs_layout_relu_drop_fwd(float* h, long n, int relu, float p, long seed, int site, hipStream_t st) {
    OCRS_CHECK_ARG(h && n > 0 && n % 4 == 0 && p >= 0.f && p < 1.f && (reinterpret_cast<uintptr_t>(h) & 15) == 0);
    hipLaunchKernelGGL(k_lay_relu_drop, dim3(lay_grid(n / 4)), dim3(256), 0, st, h, n / 4, relu, make_key(p, seed, site));
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

int ocrs_layout_relu_drop_bwd(const float* g, const float* h, float* out, long n, float p, hipStream_t st) {
    OCRS_CHECK_ARG(g && h && out && n > 0 && n % 4 == 0 && p >= 0.f && p < 1.f);
    OCRS_CHECK_ARG(((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(h) | reinterpret_cast<uintptr_t>(out)) & 15) == 0);
    hipLaunchKernelGGL(k_lay_relu_drop_bwd, dim3(lay_grid(n / 4)), dim3(256), 0, st, g, h, out, n / 4, make_key(p, 0, 0).scale);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

long ocrs_layout_col_sum_ws_floats(int C, long rows) { return (long)colsum_blocks(rows) * C; }

int ocrs_layout_col_sum(const float* a, int ld, int C, int Cout, float* out, float* ws, long rows, hipStream_t st) {
    OCRS_CHECK_ARG(a && out && ws && rows > 0 && C > 0 && C % 4 == 0 && ld % 4 == 0 && ld >= C && Cout >= 1 && Cout <= C &&
                   (reinterpret_cast<uintptr_t>(a) & 15) == 0 && (reinterpret_cast<uintptr_t>(ws) & 15) == 0);
    const int nb = colsum_blocks(rows);
    hipLaunchKernelGGL(k_lay_colsum, dim3(nb, (C + 255) / 256), dim3(256), 0, st, a, ld, C, rows, ws);
    hipLaunchKernelGGL(k_lay_colreduce, dim3((C + 63) / 64), dim3(256), 0, st, (const float*)ws, nb, C, out, Cout, (float*)nullptr, 0);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

long ocrs_layout_loss_ws_bytes(void) { return (long)(LOSS_MAXB * sizeof(LossPart) + 64); }

int ocrs_layout_loss(const float* pred, const float* target, float pos_weight, int pred_is_prob, float* loss, float* dlogits, long long* counts, void* ws,
                     long rows, hipStream_t st) {
    OCRS_CHECK_ARG(pred && target && loss && ws && rows > 0 && (reinterpret_cast<uintptr_t>(ws) & 15) == 0);
    long nb = (rows + 255) / 256;
    if (nb > LOSS_MAXB) nb = LOSS_MAXB;
    // ws: the arrival counter (one word, zero on entry, left zero) in the first 64 bytes, then the per-workgroup partials
    hipLaunchKernelGGL(k_lay_loss, dim3((int)nb), dim3(256), 0, st, pred, target, pos_weight, pred_is_prob, loss, dlogits, counts,
                       reinterpret_cast<LossPart*>(static_cast<char*>(ws) + 64), static_cast<unsigned*>(ws), rows);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

int ocrs_layout_stats_update(const long long* counts, double* sums, hipStream_t st) {
    OCRS_CHECK_ARG(counts && sums);
    hipLaunchKernelGGL(k_lay_stats_update, dim3(1), dim3(64), 0, st, counts, sums);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

int ocrs_layout_head_out(const float* logits, int ld, float* out, long rows, int probs, hipStream_t st) {
    OCRS_CHECK_ARG(logits && out && rows > 0 && ld >= 2);
    hipLaunchKernelGGL(k_lay_head_out, dim3(lay_grid(rows)), dim3(256), 0, st, logits, ld, out, rows, probs);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

int ocrs_layout_head_grad_in(const float* g, float* dlog, int ld, long rows, hipStream_t st) {
    OCRS_CHECK_ARG(g && dlog && rows > 0 && ld >= 4 && ld % 4 == 0 && (reinterpret_cast<uintptr_t>(dlog) & 15) == 0 && (reinterpret_cast<uintptr_t>(g) & 7) == 0);
    hipLaunchKernelGGL(k_lay_head_grad_in, dim3(lay_grid(rows * (ld / 4))), dim3(256), 0, st, g, dlog, ld, rows);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

int ocrs_layout_dropout_mask(unsigned char* mask, long n, float p, long seed, int site, hipStream_t st) {
    OCRS_CHECK_ARG(mask && n > 0 && p >= 0.f && p < 1.f);
    DropKey dk = make_key(p, seed, site);
    dk.on = 1;
    hipLaunchKernelGGL(k_lay_mask, dim3(lay_grid((n + 3) / 4)), dim3(256), 0, st, mask, n, dk);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

}  // extern "C"
