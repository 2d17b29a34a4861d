// The detector's input side: what torchvision 0.4.2's GeneralizedRCNNTransform does to a list of frames before the backbone sees them --
// normalise, resize so that the short side reaches min_size unless the long side would pass max_size, copy into one zero-padded batch --
// and to the targets of training: boxes scaled, masks resized through nearest.  For uint8 frames, read in place through their strides.
// DESIGN.md section 25 states the arithmetic; tests/detin_ref.py is its numpy twin.
//
// Everything that divides is computed on the host (cosypose_amd/detector_input.py, numpy float32 and Python doubles) and arrives in the one
// table of section 18: the 3 x 256 values p_c(u) = ((float32(u) / 255f) - mean_c) / std_c at its head, the axes' tap and nearest tables, the
// mask planes' units; the two box ratios of a frame ride in its descriptor.  The tap load, the two-tap sample, the nearest gather, the byte
// store and the rules for a descriptor's table offsets are image_device.h's, shared with kernels_frames.hip.  In floating point the kernel does
// section 18's three fused multiply-adds and three lone products, one product per box coordinate, and nothing else.  Scalar float32 only.
//
// One launch over a batch of frames of ANY sizes and all their masks: blockIdx.z < n is the image of frame z, every later z one mask
// plane named by the unit table.  A thread of an image unit owns DI_PX horizontally adjacent columns of one row of the PADDED image in all
// three channels: the taps, the weights and the two row addresses are shared by the channels, and it stores three 16-byte vectors where
// the row is aligned.  Inside (nh, nw) it stores the value, outside +0.0: every element of the batch is written exactly once and nothing
// has to be zeroed first.  A frame the network sees at its own size takes one tap.  The first workgroup of an image unit also scales the
// frame's boxes.  A thread of a mask unit owns DI_PX adjacent bytes and stores them as one dword where the address allows.  Every
// workgroup takes its branches uniformly, the barrier behind the load of p into LDS included.
#include "cosy_common.h"
#include "image_device.h"

namespace cosy {
namespace {

constexpr int DI_THREADS = 256, DI_LANES = 32, DI_ROWS = DI_THREADS / DI_LANES, DI_PX = IMG_PX, DI_TILE_W = DI_LANES * DI_PX;
constexpr int DI_LUT = 3 * 256;

// what both sides ask of a descriptor before anything is read or written through it: -> 0, or the number of the rule it breaks
__host__ __device__ inline int detin_item_fault(const cosy_detin_item_t& it, int Hp, int Wp, long n_tables) {
    if (it.frame == nullptr) return 1;
    if (it.h < 1 || it.w < 1 || it.nh < 1 || it.nw < 1) return 2;
    if (it.nh > Hp || it.nw > Wp) return 3;
    if (it.sc < 0 || it.sy < 0 || it.sx < 0 || it.n_masks < 0 || it.n_boxes < 0) return 4;
    const bool one_tap = (it.flags & COSY_DETIN_ONE_TAP) && it.nh == it.h && it.nw == it.w;
    if (!one_tap) {
        if (!table_inside(it.xb, 4L * it.nw, n_tables) || !table_inside(it.yb, 4L * it.nh, n_tables)) return 5;
        if (!tap_table_aligned(it.xb) || !tap_table_aligned(it.yb)) return 6;
    }
    if (it.n_masks > 0) {
        if (it.masks == nullptr || it.masks_out == nullptr) return 7;
        if (!nearest_table_ok(it.xn, it.nw, n_tables) || !nearest_table_ok(it.yn, it.nh, n_tables)) return 8;
    }
    if (it.n_boxes > 0 && (it.boxes == nullptr || it.boxes_out == nullptr)) return 9;
    return 0;
}

// the valid floats of v[] to p: one 16-byte vector where all four are there and p is 16-byte aligned
__device__ __forceinline__ void store_f4(float* p, const float* v, int n_valid) {
    if (n_valid == DI_PX && ((uintptr_t)p & 15) == 0) {
        f32x4 q;
        q.x = v[0]; q.y = v[1]; q.z = v[2]; q.w = v[3];
        *reinterpret_cast<f32x4*>(p) = q;
        return;
    }
#pragma unroll
    for (int j = 0; j < DI_PX; ++j)
        if (j < n_valid) p[j] = v[j];
}

__global__ __launch_bounds__(DI_THREADS) void detector_input_kernel(const cosy_detin_item_t* __restrict__ items, int n, int Hp, int Wp,
                                                                    const int* __restrict__ tables, long n_tables, int lut, int units,
                                                                    int n_units, float* __restrict__ out_images) {
    __shared__ float p_of[DI_LUT];
    const int z = blockIdx.z;
    const bool is_mask = z >= n;                              // block-uniform, as everything derived from z
    int i = z, plane = 0;
    if (is_mask) {
        const int u = z - n;
        if (u >= n_units) return;
        i = tables[units + 2 * (long)u];
        plane = tables[units + 2 * (long)u + 1];
        if (i < 0 || i >= n) return;                          // a unit whose item does not exist
    }
    const cosy_detin_item_t it = items[i];
    // a descriptor the kernel cannot serve leaves its outputs untouched and nothing is read through it
    if (detin_item_fault(it, Hp, Wp, n_tables)) return;
    const int y = blockIdx.y * DI_ROWS + threadIdx.x / DI_LANES;
    const int x0 = (blockIdx.x * DI_LANES + threadIdx.x % DI_LANES) * DI_PX;

    if (is_mask) {
        if (plane < 0 || plane >= it.n_masks) return;         // a unit whose plane does not exist
        if (y >= it.nh || x0 >= it.nw) return;
        const int n_valid = it.nw - x0 < DI_PX ? it.nw - x0 : DI_PX;
        const unsigned char* src = it.masks + (size_t)plane * it.h * it.w;
        unsigned px[DI_PX] = {0u, 0u, 0u, 0u};
        gather_nearest(src + (size_t)clamp_index(tables[it.yn + y], it.h - 1) * it.w, tables, it.xn + x0, it.w, n_valid, px);
        store_px4(it.masks_out + ((size_t)plane * it.nh + y) * it.nw + x0, px, n_valid);
        return;
    }

    for (int k = threadIdx.x; k < DI_LUT; k += DI_THREADS) p_of[k] = __int_as_float(tables[lut + k]);
    __syncthreads();                                          // every thread of an image unit's workgroup is here
    if (blockIdx.x == 0 && blockIdx.y == 0)                   // the frame's boxes: x * rw, y * rh, one product each
        for (int k = threadIdx.x; k < 4 * it.n_boxes; k += DI_THREADS) it.boxes_out[k] = __fmul_rn(it.boxes[k], (k & 1) ? it.rh : it.rw);
    if (y >= Hp || x0 >= Wp) return;
    const int n_valid = Wp - x0 < DI_PX ? Wp - x0 : DI_PX;
    float v[3][DI_PX];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int j = 0; j < DI_PX; ++j) v[c][j] = 0.0f;       // the padding: +0.0
    if (y < it.nh && x0 < it.nw) {
        const bool one_tap = (it.flags & COSY_DETIN_ONE_TAP) && it.nh == it.h && it.nw == it.w;
        if (one_tap) {
            const unsigned char* r0 = it.frame + (size_t)y * it.sy;
#pragma unroll
            for (int j = 0; j < DI_PX; ++j) {
                if (x0 + j < it.nw) {
                    const unsigned char* q = r0 + (size_t)(x0 + j) * it.sx;
#pragma unroll
                    for (int c = 0; c < 3; ++c) v[c][j] = p_of[c * 256 + q[(size_t)c * it.sc]];
                }
            }
        } else {
            const AxisTap ty = load_tap(tables, it.yb, y, it.h);
            const unsigned char* r0 = it.frame + (size_t)ty.i0 * it.sy;
            const unsigned char* r1 = it.frame + (size_t)ty.i1 * it.sy;
#pragma unroll
            for (int j = 0; j < DI_PX; ++j) {
                if (x0 + j < it.nw) {
                    const AxisTap tx = load_tap(tables, it.xb, x0 + j, it.w);
                    const size_t xa = (size_t)tx.i0 * it.sx, xb = (size_t)tx.i1 * it.sx;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const size_t oc = (size_t)c * it.sc;
                        const float* p = p_of + c * 256;
                        v[c][j] = two_tap(tx, ty, p[r0[oc + xa]], p[r0[oc + xb]], p[r1[oc + xa]], p[r1[oc + xb]]);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) store_f4(out_images + (((size_t)i * 3 + c) * Hp + y) * Wp + x0, v[c], n_valid);
}

}  // namespace
}  // namespace cosy

using namespace cosy;

extern "C" {

int cosy_detector_input(const cosy_detin_item_t* items_host, const cosy_detin_item_t* items, int n, int Hp, int Wp, const int* tables,
                        long n_tables, int lut, int units, int n_units, float* out_images, cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    COSY_REQUIRE(n >= 0 && n_units >= 0 && Hp >= 1 && Wp >= 1 && n_tables >= 0, "cosy_detector_input: n=%d n_units=%d Hp=%d Wp=%d n_tables=%ld", n,
                 n_units, Hp, Wp, n_tables);
    COSY_REQUIRE((long)n + n_units <= COSY_MAX_GRID_Y, "cosy_detector_input: n=%d frames and n_units=%d mask planes exceed %d per call", n, n_units,
                 COSY_MAX_GRID_Y);
    COSY_REQUIRE(cdiv(Hp, DI_ROWS) <= COSY_MAX_GRID_Y && 3L * Hp * Wp < (1L << 31), "cosy_detector_input: images of 3 x %d x %d are too large", Hp, Wp);
    COSY_REQUIRE(lut >= 0 && (long)lut + DI_LUT <= n_tables, "cosy_detector_input: lut=%d and its %d entries lie outside the %ld of tables", lut, DI_LUT,
                 n_tables);
    COSY_REQUIRE(units >= 0 && (long)units + 2L * n_units <= n_tables, "cosy_detector_input: units=%d and its %d pairs lie outside the %ld of tables",
                 units, n_units, n_tables);
    if (n == 0) return COSY_OK;
    COSY_REQUIRE_PTR("cosy_detector_input", items_host); COSY_REQUIRE_PTR("cosy_detector_input", items);
    COSY_REQUIRE_PTR("cosy_detector_input", tables); COSY_REQUIRE_PTR("cosy_detector_input", out_images);
    COSY_REQUIRE(((uintptr_t)items & 15) == 0 && ((uintptr_t)items_host & 7) == 0 && ((uintptr_t)tables & 15) == 0 && ((uintptr_t)out_images & 3) == 0,
                 "cosy_detector_input: items or tables not 16-byte, items_host not 8-byte or out_images not 4-byte aligned");
    for (int i = 0; i < n; ++i) {
        const int fault = detin_item_fault(items_host[i], Hp, Wp, n_tables);
        COSY_REQUIRE(fault == 0, "cosy_detector_input: item %d cannot be served (rule %d: 1 null frame, 2 a size < 1, 3 larger than the batch, 4 a "
                     "negative stride or count, 5 tap tables outside the %ld of tables, 6 tap tables misaligned, 7 null masks, 8 nearest tables "
                     "outside, 9 null boxes)", i, fault, n_tables);
    }
    hipLaunchKernelGGL(detector_input_kernel, dim3(cdiv(Wp, DI_TILE_W), cdiv(Hp, DI_ROWS), n + n_units), dim3(DI_THREADS), 0, s, items, n, Hp, Wp,
                       tables, n_tables, lut, units, n_units, out_images);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

}  // extern "C"
