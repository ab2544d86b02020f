// Tiled detection: the pixel work on either side of the detector's eval forward when a page is detected in overlapping
// tiles at (near) native resolution instead of being squeezed to the training size whole.
//
//   k_tile_resize_{h,v}       resize(transform_image(page[:, y0:y0+th, x0:x0+tw]), size) for every tile window of every page, cut straight
//                             from the uint8 page store (no fp32 page exists); the two passes of ocrs_resize_aa through the same
//                             aa_span / aa_dot, px_u8 per tap: same bits
//   k_binarize_resize_tiles   k_binarize_resize_pages with the owner tile's window in the place of the page: every canvas byte comes from
//                             the tile that owns its pixel (the cuts in the middle of the overlaps), padding included
//
// Both are byte-bound streaming kernels like their neighbours in input_pipe.hip and ocr_infer.hip: no LDS, no MFMA, every table stays on
// the device.  A tile is {page, y0, x0, th, tw}; a tile that does not lie inside its page (or whose page does not lie inside the store) is
// skipped by both passes, and a table entry that points outside the probabilities reads nothing: bad tables cannot move an access out of
// the buffers the caller gave.
#include "input_pipe.h"

namespace {

struct TileWin {
    const uint8_t* src;  // the window's first byte
    int W, th, tw;       // the page's row pitch, the window's size
};
// the window of tile t, or false if it is not inside page and store
__device__ __forceinline__ bool tile_window(const uint8_t* __restrict__ pages, long pages_bytes, const long long* __restrict__ page_offs,
                                            const int* __restrict__ page_sizes, int B, const int* __restrict__ tiles, int t, int max_th, TileWin& win) {
    const int p = tiles[5 * t], y0 = tiles[5 * t + 1], x0 = tiles[5 * t + 2], th = tiles[5 * t + 3], tw = tiles[5 * t + 4];
    if ((unsigned)p >= (unsigned)B) return false;
    const int H = page_sizes[2 * p], W = page_sizes[2 * p + 1];
    const long long off = page_offs[p];
    if (H < 1 || W < 1 || off < 0 || off + (long long)H * W > pages_bytes) return false;
    if (y0 < 0 || x0 < 0 || th < 1 || tw < 1 || th > max_th || y0 > H - th || x0 > W - tw) return false;
    win.src = pages + off + (size_t)y0 * W + x0;
    win.W = W, win.th = th, win.tw = tw;
    return true;
}

// uint8 windows -> ws [T][max_th][ow]: one thread per element, as k_resize_aa_h.  Neighbouring lanes read overlapping byte spans of one
// page row (L2/TA coalesces them) and store consecutive floats.
__global__ __launch_bounds__(256) void k_tile_resize_h(const uint8_t* __restrict__ pages, long pages_bytes, const long long* __restrict__ page_offs,
                                                       const int* __restrict__ page_sizes, int B, const int* __restrict__ tiles, int max_th,
                                                       float* __restrict__ ws, int ow) {
    const int ox = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, t = blockIdx.z;
    TileWin win;
    if (ox >= ow || !tile_window(pages, pages_bytes, page_offs, page_sizes, B, tiles, t, max_th, win) || y >= win.th) return;
    const AaSpan s = aa_span(ox, win.tw, (float)win.tw / (float)ow);
    ws[((size_t)t * max_th + y) * ow + ox] = aa_dot(s, win.src + (size_t)y * win.W + s.lo, 1);
}
// ws [T][max_th][ow] -> out [T][oh][ow], as k_resize_aa_v
__global__ __launch_bounds__(256) void k_tile_resize_v(const uint8_t* __restrict__ pages, long pages_bytes, const long long* __restrict__ page_offs,
                                                       const int* __restrict__ page_sizes, int B, const int* __restrict__ tiles, int max_th,
                                                       const float* __restrict__ ws, float* __restrict__ out, int oh, int ow) {
    const int ox = blockIdx.x * 256 + threadIdx.x, oy = blockIdx.y, t = blockIdx.z;
    TileWin win;
    if (ox >= ow || !tile_window(pages, pages_bytes, page_offs, page_sizes, B, tiles, t, max_th, win)) return;
    const AaSpan s = aa_span(oy, win.th, (float)win.th / (float)oh);  // uniform over the block: scalar registers
    out[((size_t)t * oh + oy) * ow + ox] = aa_dot(s, ws + ((size_t)t * max_th + s.lo) * ow + ox, ow);
}

// One lane = 16 consecutive canvas bytes, padding included, taken one canvas row at a time as in k_binarize_resize_pages.  Per row piece:
// the page's size, the tile row that owns y (the first row cut >= y) and its source row scale; then the piece is walked as runs between
// column cuts, the owner tile's window and column scale looked up once per run.  Per byte: one multiply, floorf, clamp, load, compare.
__global__ __launch_bounds__(256) void k_binarize_resize_tiles(const float* __restrict__ prob, int T, int h, int w, const int* __restrict__ tiles,
                                                               const int* __restrict__ tile_offs, const int* __restrict__ page_sizes,
                                                               const int* __restrict__ grids, const int* __restrict__ row_cuts,
                                                               const int* __restrict__ col_cuts, int K, uint8_t* __restrict__ out, int Hmax, int Wmax,
                                                               long total, float threshold) {
    const long nchunks = (total + 15) / 16;
    for (long c = (long)blockIdx.x * 256 + threadIdx.x; c < nchunks; c += (long)gridDim.x * 256) {
        const long e = c * 16;
        long row = e / Wmax;  // b * Hmax + y
        int x = (int)(e - row * Wmax);
        long b = row / Hmax;
        int y = (int)(row - b * Hmax);
        const int nv = (int)min(16L, total - e);
        unsigned long long lo = 0ULL, hi = 0ULL;  // bytes 0..7 and 8..15
        for (int k = 0; k < nv;) {
            const int run = min(nv - k, Wmax - x);  // the piece of row (b, y) from x on
            const int H = min(page_sizes[2 * b], Hmax), W = min(page_sizes[2 * b + 1], Wmax);
            if (y < H && x < W) {
                const int ny = min(max(grids[2 * b], 1), K), nx = min(max(grids[2 * b + 1], 1), K);
                const int* rc = row_cuts + b * K;
                const int* cc = col_cuts + b * K;
                int iy = 0, ix = 0;
                while (iy < ny - 1 && rc[iy] < y) ++iy;  // the last tile of an axis owns whatever the cuts before it do not
                const long t0 = (long)tile_offs[b] + (long)iy * nx;
                const int last = x + min(run, W - x) - 1;  // the piece's last column inside the page
                for (int xx = x; xx <= last;) {
                    while (ix < nx - 1 && cc[ix] < xx) ++ix;
                    const int end = ix < nx - 1 ? min(cc[ix], last) : last;  // >= xx
                    const long t = t0 + ix;
                    if (t >= 0 && t < T) {
                        const int y0 = tiles[5 * t + 1], x0 = tiles[5 * t + 2], th = max(tiles[5 * t + 3], 1), tw = max(tiles[5 * t + 4], 1);
                        const float sy = (float)h / (float)th, sx = (float)w / (float)tw;
                        const float* src = prob + (t * h + max(min((int)floorf((float)(y - y0) * sy), h - 1), 0)) * (long)w;
                        for (int xq = xx; xq <= end; ++xq) {
                            const int xs = max(min((int)floorf((float)(xq - x0) * sx), w - 1), 0);
                            if (src[xs] > threshold) {
                                const int bit = 8 * (k + xq - x);
                                if (bit < 64) lo |= 1ULL << bit; else hi |= 1ULL << (bit - 64);
                            }
                        }
                    }
                    xx = end + 1;
                }
            }
            k += run, x += run;
            if (x == Wmax) {
                x = 0;
                if (++y == Hmax) y = 0, ++b;
            }
        }
        if (nv == 16) {
            *reinterpret_cast<uint4*>(out + e) = make_uint4((unsigned)lo, (unsigned)(lo >> 32), (unsigned)hi, (unsigned)(hi >> 32));
        } else {
            for (int k = 0; k < nv; ++k) out[e + k] = (uint8_t)(((k < 8 ? lo >> (8 * k) : hi >> (8 * (k - 8)))) & 0xff);
        }
    }
}

}  // namespace

extern "C" {

long ocrs_tile_batch_ws_floats(int T, int max_th, int ow) { return T > 0 && max_th > 0 && ow > 0 ? (long)T * max_th * ow : 0; }

int ocrs_tile_batch(const unsigned char* pages, long pages_bytes, const long long* page_offs, const int* page_sizes, int B, const int* tiles, int T, int max_th,
                    float* ws, long ws_floats, float* out, int oh, int ow, hipStream_t st) {
    OCRS_CHECK_ARG(B >= 0 && T >= 0 && T <= 65535 && pages_bytes >= 0 && max_th > 0 && max_th <= 65535 && oh > 0 && oh <= 65535 && ow > 0);
    if (T == 0) return OCRS_OK;
    OCRS_CHECK_ARG(pages && page_offs && page_sizes && tiles && ws && out && ws_floats >= ocrs_tile_batch_ws_floats(T, max_th, ow));
    const unsigned gx = (unsigned)((ow + 255) / 256);
    hipLaunchKernelGGL(k_tile_resize_h, dim3(gx, max_th, T), dim3(256), 0, st, pages, pages_bytes, page_offs, page_sizes, B, tiles, max_th, ws, ow);
    hipLaunchKernelGGL(k_tile_resize_v, dim3(gx, oh, T), dim3(256), 0, st, pages, pages_bytes, page_offs, page_sizes, B, tiles, max_th, (const float*)ws, out, oh,
                       ow);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

int ocrs_binarize_resize_tiles(const float* prob, int T, int h, int w, const int* tiles, const int* tile_offs, const int* page_sizes, const int* grids,
                               const int* row_cuts, const int* col_cuts, int max_axis, unsigned char* out, int B, int Hmax, int Wmax, float threshold,
                               hipStream_t st) {
    OCRS_CHECK_ARG(B >= 0 && T >= 0 && h > 0 && w > 0 && Hmax > 0 && Wmax > 0 && max_axis >= 1 && max_axis <= OCRS_TILES_AXIS_MAX);
    const long total = (long)B * Hmax * Wmax;
    if (total == 0) return OCRS_OK;
    OCRS_CHECK_ARG(prob && tiles && tile_offs && page_sizes && grids && row_cuts && col_cuts && out && aligned16(out));
    long g = ((total + 15) / 16 + 255) / 256;
    g = g > kNumCU * 8 ? kNumCU * 8 : g;
    hipLaunchKernelGGL(k_binarize_resize_tiles, dim3((unsigned)g), dim3(256), 0, st, prob, T, h, w, tiles, tile_offs, page_sizes, grids, row_cuts, col_cuts, max_axis,
                       out, Hmax, Wmax, total, threshold);
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

}  // extern "C"
