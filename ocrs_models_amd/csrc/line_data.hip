// Recognition training data (ocrs_models/datasets/hiertext.py:238-274): the line crops of the dataset live in HBM as one packed uint8
// buffer (Python: ocrs_models_amd/datasets.py); a batch is gathered from it and every crop's polygon mask is rasterised next to it.
//   k_line_mask    generate_mask(w, h, [poly], shrink_dist=0.0) = PIL's ImageDraw.polygon(poly, fill="white", outline=None) on a mode "1"
//                  image, restated operation by operation (tests/hiertext_ref.py is the host restatement this was ported from)
//   k_line_batch   the same plus the coalesced byte copy of the crop, for B store indices, in the packed layout ocrs_augment_lines reads
// One 64-lane workgroup per (sample, row).  PIL's fill is a sequential scanline algorithm whose result depends on the edge order, so lane 0
// builds and sorts the row's crossings in LDS exactly in that order (csrc/poly_fill.h, shared with csrc/page_data.hip); then all lanes
// write the row's bytes.  No atomics, no allocation.
#include "poly_fill.h"

#pragma clang fp contract(off)  // PIL's edge arithmetic rounds after every operation (csrc/poly_fill.h says the same for its own text)

namespace {

__global__ __launch_bounds__(64) void k_line_mask(const int* __restrict__ verts, const long long* __restrict__ vert_offs,
                                                  const int* __restrict__ vert_counts, const int* __restrict__ sizes,
                                                  const long long* __restrict__ out_offs, uint8_t* __restrict__ out) {
    __shared__ RowScratch s;
    const int b = blockIdx.y, y = blockIdx.x;
    const int H = sizes[2 * b], W = sizes[2 * b + 1];
    if (y >= H) return;
    mask_row(s, verts + 2 * vert_offs[b], vert_counts[b], H, W, y, out + out_offs[b] + (long long)y * W);
}

// batch_offs [B][3]: the offsets ocrs_augment_lines takes; element 0 = where the sample's crop (and mask) starts in the packed batch
__global__ __launch_bounds__(64) void k_line_batch(const uint8_t* __restrict__ pixels, const long long* __restrict__ px_offs,
                                                   const int* __restrict__ sizes, const int* __restrict__ verts,
                                                   const long long* __restrict__ vert_offs, const int* __restrict__ vert_counts, int N,
                                                   const int* __restrict__ indices, const long long* __restrict__ batch_offs,
                                                   uint8_t* __restrict__ crops, uint8_t* __restrict__ masks) {
    __shared__ RowScratch s;
    const int b = blockIdx.y, y = blockIdx.x;
    int l = indices[b];
    l = l < 0 ? 0 : (l >= N ? N - 1 : l);  // (indices are checked on the host; never read outside the store)
    const int H = sizes[2 * l], W = sizes[2 * l + 1];
    if (y >= H) return;
    const long long at = batch_offs[3 * b] + (long long)y * W;
    const uint8_t* src = pixels + px_offs[l] + (long long)y * W;
    uint8_t* dst = crops + at;
    if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {  // 16 bytes per lane where the row allows it
        const int nv = W >> 4;
        for (int i = threadIdx.x; i < nv; i += 64) reinterpret_cast<uint4*>(dst)[i] = reinterpret_cast<const uint4*>(src)[i];
        for (int x = (nv << 4) + threadIdx.x; x < W; x += 64) dst[x] = src[x];
    } else {
        for (int x = threadIdx.x; x < W; x += 64) dst[x] = src[x];
    }
    mask_row(s, verts + 2 * vert_offs[l], vert_counts[l], H, W, y, masks + at);
}

}  // namespace

extern "C" {

int ocrs_line_mask(const int* vertices, const long long* vertex_offs, const int* vertex_counts, const int* sizes, const long long* out_offs,
                   void* out_u8, int n, int max_h, hipStream_t st) {
    OCRS_CHECK_ARG(n >= 0 && n <= 65535);
    if (n == 0) return OCRS_OK;
    OCRS_CHECK_ARG(vertices && vertex_offs && vertex_counts && sizes && out_offs && out_u8 && max_h >= 1 && max_h <= 65535);
    hipLaunchKernelGGL(k_line_mask, dim3(max_h, n), dim3(64), 0, st, vertices, vertex_offs, vertex_counts, sizes, out_offs,
                       static_cast<uint8_t*>(out_u8));
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

int ocrs_line_batch(const void* pixels_u8, const long long* pixel_offs, const int* sizes, const int* vertices, const long long* vertex_offs,
                    const int* vertex_counts, int N, const int* indices, int B, int max_h, const long long* batch_offs, void* out_crops_u8,
                    void* out_masks_u8, hipStream_t st) {
    OCRS_CHECK_ARG(B >= 0 && B <= 65535 && N >= 1);
    if (B == 0) return OCRS_OK;
    OCRS_CHECK_ARG(pixels_u8 && pixel_offs && sizes && vertices && vertex_offs && vertex_counts && indices && batch_offs && out_crops_u8 &&
                   out_masks_u8 && max_h >= 1 && max_h <= 65535);
    hipLaunchKernelGGL(k_line_batch, dim3(max_h, B), dim3(64), 0, st, static_cast<const uint8_t*>(pixels_u8), pixel_offs, sizes, vertices,
                       vertex_offs, vertex_counts, N, indices, batch_offs, static_cast<uint8_t*>(out_crops_u8),
                       static_cast<uint8_t*>(out_masks_u8));
    OCRS_LAUNCH_CHECK();
    return OCRS_OK;
}

}  // extern "C"
