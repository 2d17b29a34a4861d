// The frames' own resize: what CropResizeToAspectAugmentation.__call__ of the reference (cosypose/datasets/augmentations.py:137-192) does to
// a frame of the target aspect that is not yet at the training size -- the image through float32 bilinear interpolation with half-pixel
// centres (F.interpolate, align_corners=False) and a truncating cast to bytes, the instance mask through nearest.  DESIGN.md section 18
// states the arithmetic; tests/frames_ref.py is its numpy twin.
//
// Everything that divides is computed on the host (cosypose_amd/frames.py, numpy float32) and arrives in one table: per axis and output
// index i0, i1, l0, l1 (the two taps and their float32 weights) and the nearest source index, and the 256 values float32(u) / 255f.  The
// kernel does the three fused multiply-adds and the three lone products of section 18 and nothing else in floating point: fmaf and
// __fmul_rn, so that nothing is contracted or reassociated.  Scalar float32 only.
//
// One launch over a batch of frames of ANY sizes (a per-frame descriptor names the sources and the tables of its two axes).  A thread
// owns FR_PX horizontally adjacent output bytes of one plane and stores them as one dword where the address allows; it reads its row's
// taps and weights once.  blockIdx.z = frame * 4 + plane: planes 0-2 are the image's channels, plane 3 is the mask.  Every workgroup
// takes its branches uniformly.  A frame already at (H, W) is copied.  No workspace: both passes are two-tap.
#include "cosy_common.h"

namespace cosy {
namespace {

constexpr int FR_THREADS = 256, FR_LANES = 32, FR_ROWS = FR_THREADS / FR_LANES, FR_PX = 4, FR_TILE_W = FR_LANES * FR_PX;
constexpr int FR_PLANES = 4;                                 // three channels and the mask
constexpr int FR_LUT = 256;

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }

// the valid bytes of px[] to p: one dword where all four are there and p is 4-byte aligned
__device__ __forceinline__ void store_px4(unsigned char* p, const unsigned* px, int n_valid) {
    if (n_valid == FR_PX && ((uintptr_t)p & 3) == 0) {
        *reinterpret_cast<unsigned*>(p) = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
        return;
    }
#pragma unroll
    for (int j = 0; j < FR_PX; ++j)
        if (j < n_valid) p[j] = (unsigned char)px[j];
}

__global__ __launch_bounds__(FR_THREADS) void resize_frames_kernel(const cosy_frame_item_t* __restrict__ items, int H, int W,
                                                                   const int* __restrict__ tables, long n_tables, int lut,
                                                                   unsigned char* __restrict__ out_images,
                                                                   unsigned char* __restrict__ out_masks) {
    __shared__ float p_of[FR_LUT];
    const int i = blockIdx.z / FR_PLANES, plane = blockIdx.z % FR_PLANES;
    const cosy_frame_item_t it = items[i];
    const bool is_mask = plane == FR_PLANES - 1;
    const unsigned char* src = is_mask ? it.mask : it.image;
    // a descriptor the kernel cannot serve leaves its frame of the outputs untouched and nothing is read through it
    if (src == nullptr || it.h < 1 || it.w < 1 || (is_mask && out_masks == nullptr)) return;
    const bool copy = it.h == H && it.w == W;
    if (!copy) {
        const long xo = is_mask ? it.xn : it.xb, yo = is_mask ? it.yn : it.yb, per = is_mask ? 1 : 4;
        if (xo < 0 || yo < 0 || xo + per * W > n_tables || yo + per * H > n_tables) return;
        if (!is_mask && ((xo | yo) & 3)) return;              // the tap tables are read as 16-byte entries
    }
    const bool interpolate = !copy && !is_mask;
    if (interpolate) {                                        // block-uniform: every thread of the workgroup reaches the barrier
        p_of[threadIdx.x] = __int_as_float(tables[lut + threadIdx.x]);
        __syncthreads();
    }
    const int y = blockIdx.y * FR_ROWS + threadIdx.x / FR_LANES;
    const int x0 = (blockIdx.x * FR_LANES + threadIdx.x % FR_LANES) * FR_PX;
    if (y >= H || x0 >= W) return;
    const int n_valid = W - x0 < FR_PX ? W - x0 : FR_PX;
    unsigned px[FR_PX] = {0u, 0u, 0u, 0u};
    unsigned char* dst;
    if (is_mask) {
        dst = out_masks + ((size_t)i * H + y) * W + x0;
        const int sy = copy ? y : clampi(tables[it.yn + y], it.h - 1);
        const unsigned char* row = src + (size_t)sy * it.w;
#pragma unroll
        for (int j = 0; j < FR_PX; ++j)
            if (j < n_valid) px[j] = row[copy ? x0 + j : clampi(tables[it.xn + x0 + j], it.w - 1)];
    } else {
        dst = out_images + (((size_t)i * 3 + plane) * H + y) * W + x0;
        const unsigned char* img = src + (size_t)plane * it.h * it.w;
        if (copy) {
#pragma unroll
            for (int j = 0; j < FR_PX; ++j)
                if (j < n_valid) px[j] = img[(size_t)y * W + x0 + j];
        } else {
            const int4 ty = *reinterpret_cast<const int4*>(tables + it.yb + 4 * (size_t)y);
            const unsigned char* r0 = img + (size_t)clampi(ty.x, it.h - 1) * it.w;
            const unsigned char* r1 = img + (size_t)clampi(ty.y, it.h - 1) * it.w;
            const float ly0 = __int_as_float(ty.z), ly1 = __int_as_float(ty.w);
#pragma unroll
            for (int j = 0; j < FR_PX; ++j) {
                if (j < n_valid) {
                    const int4 tx = *reinterpret_cast<const int4*>(tables + it.xb + 4 * (size_t)(x0 + j));
                    const int xa = clampi(tx.x, it.w - 1), xb = clampi(tx.y, it.w - 1);
                    const float lx0 = __int_as_float(tx.z), lx1 = __int_as_float(tx.w);
                    const float top = fmaf(lx0, p_of[r0[xa]], __fmul_rn(lx1, p_of[r0[xb]]));
                    const float bot = fmaf(lx0, p_of[r1[xa]], __fmul_rn(lx1, p_of[r1[xb]]));
                    const float v = fmaf(ly0, top, __fmul_rn(ly1, bot));
                    px[j] = (unsigned)(int)__fmul_rn(v, 255.0f) & 255u;       // (uint8) of the truncated product
                }
            }
        }
    }
    store_px4(dst, px, n_valid);
}

}  // namespace
}  // namespace cosy

using namespace cosy;

extern "C" {

int cosy_resize_frames_u8(const cosy_frame_item_t* items, int n, int H, int W, const int* tables, long n_tables, int lut,
                          unsigned char* out_images, unsigned char* out_masks, cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    COSY_REQUIRE(n >= 0 && H >= 1 && W >= 1 && n_tables >= 0, "cosy_resize_frames_u8: n=%d H=%d W=%d n_tables=%ld", n, H, W, n_tables);
    COSY_REQUIRE((long)n * FR_PLANES <= COSY_MAX_GRID_Y, "cosy_resize_frames_u8: n=%d exceeds %d frames per call", n, COSY_MAX_GRID_Y / FR_PLANES);
    COSY_REQUIRE(cdiv(H, FR_ROWS) <= COSY_MAX_GRID_Y && 3L * H * W < (1L << 31), "cosy_resize_frames_u8: frames of 3 x %d x %d are too large", H, W);
    COSY_REQUIRE(lut >= 0 && (long)lut + FR_LUT <= n_tables, "cosy_resize_frames_u8: lut=%d and its %d entries lie outside the %ld of tables", lut,
                 FR_LUT, n_tables);
    if (n == 0) return COSY_OK;
    COSY_REQUIRE_PTR("cosy_resize_frames_u8", items); COSY_REQUIRE_PTR("cosy_resize_frames_u8", tables);
    COSY_REQUIRE_PTR("cosy_resize_frames_u8", out_images);
    COSY_REQUIRE(((uintptr_t)items & 7) == 0 && ((uintptr_t)tables & 15) == 0, "cosy_resize_frames_u8: items not 8-byte or tables not 16-byte aligned");
    hipLaunchKernelGGL(resize_frames_kernel, dim3(cdiv(W, FR_TILE_W), cdiv(H, FR_ROWS), n * FR_PLANES), dim3(FR_THREADS), 0, s, items, H, W, tables,
                       n_tables, lut, out_images, out_masks);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

}  // extern "C"
