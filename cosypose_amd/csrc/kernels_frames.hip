// The frames' own resize: what CropResizeToAspectAugmentation.__call__ of the reference (cosypose/datasets/augmentations.py:137-192) does to
// a frame of the target aspect that is not yet at the training size -- the image through float32 bilinear interpolation with half-pixel
// centres (F.interpolate, align_corners=False) and a truncating cast to bytes, the instance mask through nearest.  DESIGN.md section 18
// states the arithmetic; tests/frames_ref.py is its numpy twin.
//
// Everything that divides is computed on the host (cosypose_amd/frames.py, numpy float32) and arrives in the one table of section 18,
// the 256 values float32(u) / 255f at its head.  The tap load, the two-tap sample, the nearest gather, the byte store and the test of a
// descriptor's table offsets are image_device.h's, shared with kernels_detin.hip.  In floating point the kernel does section 18's three
// fused multiply-adds and four lone products and nothing else: fmaf and __fmul_rn, nothing contracted or reassociated.  Scalar float32 only.
//
// One launch over a batch of frames of ANY sizes (a per-frame descriptor names the sources and the tables of its two axes).  A thread
// owns FR_PX horizontally adjacent output bytes of one plane and stores them as one dword where the address allows; it reads its row's
// taps and weights once.  blockIdx.z = frame * 4 + plane: planes 0-2 are the image's channels, plane 3 is the mask.  Every workgroup
// takes its branches uniformly.  A frame already at (H, W) is copied.  No workspace: both passes are two-tap.
#include "cosy_common.h"
#include "image_device.h"

namespace cosy {
namespace {

constexpr int FR_THREADS = 256, FR_LANES = 32, FR_ROWS = FR_THREADS / FR_LANES, FR_PX = IMG_PX, FR_TILE_W = FR_LANES * FR_PX;
constexpr int FR_PLANES = 4;                                 // three channels and the mask
constexpr int FR_LUT = 256;

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
    if (!copy && !(is_mask ? nearest_table_ok(it.xn, W, n_tables) && nearest_table_ok(it.yn, H, n_tables)
                           : tap_table_ok(it.xb, W, n_tables) && tap_table_ok(it.yb, H, n_tables)))
        return;
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
    const unsigned char* img = is_mask ? src : src + (size_t)plane * it.h * it.w;            // this plane of the source
    unsigned char* dst = is_mask ? out_masks + ((size_t)i * H + y) * W + x0 : out_images + (((size_t)i * 3 + plane) * H + y) * W + x0;
    if (copy) {
#pragma unroll
        for (int j = 0; j < FR_PX; ++j)
            if (j < n_valid) px[j] = img[(size_t)y * W + x0 + j];
    } else if (is_mask) {
        gather_nearest(img + (size_t)clamp_index(tables[it.yn + y], it.h - 1) * it.w, tables, it.xn + x0, it.w, n_valid, px);
    } else {
        const AxisTap ty = load_tap(tables, it.yb, y, it.h);
        const unsigned char* r0 = img + (size_t)ty.i0 * it.w;
        const unsigned char* r1 = img + (size_t)ty.i1 * it.w;
#pragma unroll
        for (int j = 0; j < FR_PX; ++j) {
            if (j < n_valid) {
                const AxisTap tx = load_tap(tables, it.xb, x0 + j, it.w);
                const float v = two_tap(tx, ty, p_of[r0[tx.i0]], p_of[r0[tx.i1]], p_of[r1[tx.i0]], p_of[r1[tx.i1]]);
                px[j] = (unsigned)(int)__fmul_rn(v, 255.0f) & 255u;           // (uint8) of the truncated product
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
