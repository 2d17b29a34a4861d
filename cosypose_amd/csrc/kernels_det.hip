// Detection side of the evaluation and of the datasets' annotations: per-instance pixel counts and boxes of instance-id masks
// (cosypose/datasets/utils.py:27-40 make_detections_from_segmentation, wrappers/visibility_wrapper.py, pose_dataset.py:90-105),
// per-object binary masks (detection_dataset.py:61-80) and box IoU with torchvision.ops.box_iou's arithmetic
// (evaluation/meters/detection_meters.py:31-35).  DESIGN.md section 16 states the contract; tests/det_ref.py is the numpy twin.
//
//   det_stats_init_kernel    stats <- 0, INT_MAX, INT_MAX, -1, -1
//   det_stats_kernel<T>      ONE pass over the masks.  A workgroup owns 1024 consecutive 16-byte slots (16384 pixels) of one image's plane, a thread
//                            reads a slot with one 16-byte load (slots are aligned in MEMORY, whatever the plane's base address and W: the
//                            first and last slot of a plane are read element by element, only where they lie inside it), cuts it into
//                            runs of equal id on one row and adds every run to an LDS table with integer atomics (add, min, max); the
//                            touched entries are flushed with integer global atomics.
//   det_stats_finish_kernel  rows that nobody touched: x1 = y1 = -1
//   det_instance_masks_kernel<T, V>   out[n] = masks[row_image[n]] == row_id[n], V = 16 pixels per thread where both planes allow it
//   det_iou_pairs_kernel / det_iou_matrix_kernel
// No floating-point atomics anywhere and integer add / min / max commute: equal inputs give equal bytes.  The IoU is written with
// one rounding per operation; the file is compiled with contraction off (the pragma below and -ffp-contract=off in build.FILE_FLAGS).
#include <limits.h>
#include "cosy_common.h"
#include "det_device.h"

#pragma clang fp contract(off)

namespace cosy {
namespace {

constexpr int DET_THREADS = 256;
constexpr int DET_SLOT_BYTES = 16;
constexpr int DET_MAX_IDS = 1024;
constexpr int DET_SLOTS_PER_THREAD_U8 = 4;                       // 64 pixels per thread, 16384 per workgroup, for both element types

__global__ __launch_bounds__(DET_THREADS) void det_stats_init_kernel(int* __restrict__ stats, long rows) {
    const long r = (long)blockIdx.x * DET_THREADS + threadIdx.x;
    if (r >= rows) return;
    int* o = stats + r * 5;
    o[0] = 0; o[1] = INT_MAX; o[2] = INT_MAX; o[3] = -1; o[4] = -1;
}

__global__ __launch_bounds__(DET_THREADS) void det_stats_finish_kernel(int* __restrict__ stats, long rows) {
    const long r = (long)blockIdx.x * DET_THREADS + threadIdx.x;
    if (r >= rows) return;
    int* o = stats + r * 5;
    if (o[0] == 0) { o[1] = -1; o[2] = -1; }
}

struct DetTable {                                                // one workgroup's partial statistics
    int count[DET_MAX_IDS], x1[DET_MAX_IDS], y1[DET_MAX_IDS], x2[DET_MAX_IDS], y2[DET_MAX_IDS];
};

__device__ __forceinline__ int det_peek(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// pixels [xa, xb] of row y hold `id`.  The plain reads only save atomics: a bound never moves back, so a read that says "already
// covered" stays true, and one that says "not covered" is followed by the atomic, which decides.
__device__ __forceinline__ void det_add_run(DetTable& t, int id, int n_ids, int y, int xa, int xb) {
    if ((unsigned)id >= (unsigned)n_ids) return;
    atomicAdd(&t.count[id], xb - xa + 1);
    if (xa < det_peek(&t.x1[id])) atomicMin(&t.x1[id], xa);
    if (xb > det_peek(&t.x2[id])) atomicMax(&t.x2[id], xb);
    if (y < det_peek(&t.y1[id])) atomicMin(&t.y1[id], y);
    if (y > det_peek(&t.y2[id])) atomicMax(&t.y2[id], y);
}

template <typename T>
__global__ __launch_bounds__(DET_THREADS) void det_stats_kernel(const T* __restrict__ masks, int n_ids, int W, int plane, int* __restrict__ stats) {
    constexpr int PX = DET_SLOT_BYTES / (int)sizeof(T);          // pixels per slot
    constexpr int SPT = DET_SLOTS_PER_THREAD_U8 * (int)sizeof(T);
    __shared__ DetTable t;
    const int b = blockIdx.y;
    for (int i = threadIdx.x; i < n_ids; i += DET_THREADS) { t.count[i] = 0; t.x1[i] = INT_MAX; t.y1[i] = INT_MAX; t.x2[i] = -1; t.y2[i] = -1; }
    __syncthreads();
    const T* base = masks + (size_t)b * plane;
    const int mis = (int)(((uintptr_t)base & (DET_SLOT_BYTES - 1)) / sizeof(T));   // elements between the slot boundary below `base` and `base`
    const int n_slots = (mis + plane + PX - 1) / PX;
    const int slot0 = blockIdx.x * (DET_THREADS * SPT) + threadIdx.x;
    for (int k = 0; k < SPT; ++k) {
        const int s = slot0 + k * DET_THREADS;
        if (s >= n_slots) break;
        const int first = s * PX - mis;                           // plane index of the slot's element 0 (negative in slot 0 when mis > 0)
        int v[PX];
        const int j0 = first < 0 ? -first : 0;
        const int j1 = plane - first < PX ? plane - first : PX;   // elements [j0, j1) of the slot lie in the plane
        if (j0 == 0 && j1 == PX) {
            const uint4 w = *reinterpret_cast<const uint4*>(base + first);
            const unsigned q[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int j = 0; j < PX; ++j) v[j] = sizeof(T) == 1 ? (int)((q[j / 4] >> (8 * (j % 4))) & 255u) : (int)q[j % 4];
        } else {
#pragma unroll
            for (int j = 0; j < PX; ++j) v[j] = (j >= j0 && j < j1) ? (int)base[first + j] : -1;
        }
        const int at = first + j0;
        int y = at / W, x = at - y * W;
        int run_id = -1, run_x = 0;
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            if (j < j0 || j >= j1) continue;
            if (v[j] != run_id) {
                if (run_id >= 0) det_add_run(t, run_id, n_ids, y, run_x, x - 1);
                run_id = v[j]; run_x = x;
            }
            if (++x == W) {                                       // a run ends with its row
                if (run_id >= 0) det_add_run(t, run_id, n_ids, y, run_x, W - 1);
                run_id = -1; x = 0; ++y;
            }
        }
        if (run_id >= 0) det_add_run(t, run_id, n_ids, y, run_x, x - 1);
    }
    __syncthreads();
    int* out = stats + (size_t)b * n_ids * 5;
    for (int i = threadIdx.x; i < n_ids; i += DET_THREADS) {
        const int c = t.count[i];
        if (c == 0) continue;
        atomicAdd(&out[i * 5 + 0], c);
        atomicMin(&out[i * 5 + 1], t.x1[i]);
        atomicMin(&out[i * 5 + 2], t.y1[i]);
        atomicMax(&out[i * 5 + 3], t.x2[i]);
        atomicMax(&out[i * 5 + 4], t.y2[i]);
    }
}

// V pixels per thread (V = 16 where the plane is a multiple of 16 pixels and masks and out are 16-byte aligned, else 1).
template <typename T, int V>
__global__ __launch_bounds__(DET_THREADS) void det_instance_masks_kernel(const T* __restrict__ masks, const int* __restrict__ row_image,
                                                                         const int* __restrict__ row_id, int B, long plane,
                                                                         unsigned char* __restrict__ out) {
    const int n = blockIdx.y;
    const long at = ((long)blockIdx.x * DET_THREADS + threadIdx.x) * V;
    if (at >= plane) return;
    const int im = row_image[n], id = row_id[n];
    unsigned char* o = out + (size_t)n * plane + at;
    const bool ok = im >= 0 && im < B;
    if (V == 1) {
        o[0] = ok ? (unsigned char)((int)masks[(size_t)im * plane + at] == id) : (unsigned char)0;
        return;
    }
    unsigned r[4] = {0u, 0u, 0u, 0u};
    if (ok) {
        const T* in = masks + (size_t)im * plane + at;
        if (sizeof(T) == 1) {
            const uint4 w = *reinterpret_cast<const uint4*>(in);
            const unsigned q[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int j = 0; j < 16; ++j) r[j / 4] |= (unsigned)((int)((q[j / 4] >> (8 * (j % 4))) & 255u) == id) << (8 * (j % 4));
        } else {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const uint4 w = reinterpret_cast<const uint4*>(in)[g];
                r[g] = (unsigned)((int)w.x == id) | ((unsigned)((int)w.y == id) << 8) | ((unsigned)((int)w.z == id) << 16) | ((unsigned)((int)w.w == id) << 24);
            }
        }
    }
    *reinterpret_cast<uint4*>(o) = make_uint4(r[0], r[1], r[2], r[3]);
}

// (Box and box_iou: det_device.h, shared with the NMS of kernels_detpost.hip)
template <bool ALIGNED>
__device__ __forceinline__ Box load_box(const float* __restrict__ p, long n) {
    if (ALIGNED) {
        const float4 v = reinterpret_cast<const float4*>(p)[n];
        return {v.x, v.y, v.z, v.w};
    }
    return cosy::load_box(p, (size_t)n);                           // the scalar form of det_device.h
}

template <bool ALIGNED>
__global__ __launch_bounds__(DET_THREADS) void det_iou_pairs_kernel(const float* __restrict__ a, const float* __restrict__ b, int N,
                                                                    float* __restrict__ iou) {
    const int n = blockIdx.x * DET_THREADS + threadIdx.x;
    if (n >= N) return;
    iou[n] = box_iou(load_box<ALIGNED>(a, n), load_box<ALIGNED>(b, n));
}

template <bool ALIGNED>
__global__ __launch_bounds__(DET_THREADS) void det_iou_matrix_kernel(const float* __restrict__ a, const float* __restrict__ b, int N, int M,
                                                                     float* __restrict__ iou) {
    const long at = (long)blockIdx.x * DET_THREADS + threadIdx.x;
    if (at >= (long)N * M) return;
    const long i = at / M, j = at - i * M;
    iou[at] = box_iou(load_box<ALIGNED>(a, i), load_box<ALIGNED>(b, j));
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace
}  // namespace cosy

using namespace cosy;

extern "C" {

int cosy_mask_instance_stats(const void* masks, int dtype, int B, int H, int W, int n_ids, int* stats, cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    COSY_REQUIRE(dtype == COSY_MASK_U8 || dtype == COSY_MASK_I32, "cosy_mask_instance_stats: dtype=%d is neither COSY_MASK_U8 nor COSY_MASK_I32", dtype);
    COSY_REQUIRE(B >= 0 && H > 0 && W > 0, "cosy_mask_instance_stats: B=%d H=%d W=%d", B, H, W);
    COSY_REQUIRE(n_ids >= 1 && n_ids <= DET_MAX_IDS, "cosy_mask_instance_stats: n_ids=%d outside [1, %d]", n_ids, DET_MAX_IDS);
    COSY_REQUIRE(B <= COSY_MAX_GRID_Y, "cosy_mask_instance_stats: B=%d exceeds %d images per call", B, COSY_MAX_GRID_Y);
    COSY_REQUIRE((long)H * W < (1L << 30), "cosy_mask_instance_stats: a frame of %d x %d is too large", H, W);
    if (B == 0) return COSY_OK;
    COSY_REQUIRE_PTR("cosy_mask_instance_stats", masks); COSY_REQUIRE_PTR("cosy_mask_instance_stats", stats);
    COSY_REQUIRE(dtype == COSY_MASK_U8 || ((uintptr_t)masks & 3) == 0, "cosy_mask_instance_stats: int32 masks not 4-byte aligned");
    const int plane = H * W;
    const long rows = (long)B * n_ids;
    hipLaunchKernelGGL(det_stats_init_kernel, dim3(cdiv(rows, DET_THREADS)), dim3(DET_THREADS), 0, s, stats, rows);
    COSY_CHECK_HIP(hipGetLastError());
    const int px_per_group = DET_THREADS * DET_SLOTS_PER_THREAD_U8 * DET_SLOT_BYTES;       // pixels a workgroup covers, for both types
    const int groups = cdiv((long)plane + DET_SLOT_BYTES, px_per_group);                    // (+ one slot: a plane that starts inside a slot)
    if (dtype == COSY_MASK_U8) {
        hipLaunchKernelGGL(det_stats_kernel<unsigned char>, dim3(groups, B), dim3(DET_THREADS), 0, s, (const unsigned char*)masks, n_ids, W, plane, stats);
    } else {
        hipLaunchKernelGGL(det_stats_kernel<int>, dim3(groups, B), dim3(DET_THREADS), 0, s, (const int*)masks, n_ids, W, plane, stats);
    }
    COSY_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(det_stats_finish_kernel, dim3(cdiv(rows, DET_THREADS)), dim3(DET_THREADS), 0, s, stats, rows);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

int cosy_instance_masks(const void* masks, int dtype, const int* row_image, const int* row_id, int B, int H, int W, int N, unsigned char* out,
                        cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    COSY_REQUIRE(dtype == COSY_MASK_U8 || dtype == COSY_MASK_I32, "cosy_instance_masks: dtype=%d is neither COSY_MASK_U8 nor COSY_MASK_I32", dtype);
    COSY_REQUIRE(B >= 0 && N >= 0 && H > 0 && W > 0, "cosy_instance_masks: B=%d N=%d H=%d W=%d", B, N, H, W);
    COSY_REQUIRE(N <= COSY_MAX_GRID_Y, "cosy_instance_masks: N=%d exceeds %d rows per call", N, COSY_MAX_GRID_Y);
    COSY_REQUIRE((long)H * W < (1L << 30), "cosy_instance_masks: a frame of %d x %d is too large", H, W);
    if (N == 0) return COSY_OK;
    COSY_REQUIRE_PTR("cosy_instance_masks", row_image); COSY_REQUIRE_PTR("cosy_instance_masks", row_id); COSY_REQUIRE_PTR("cosy_instance_masks", out);
    COSY_REQUIRE(B == 0 || masks != nullptr, "cosy_instance_masks: null masks");
    COSY_REQUIRE(dtype == COSY_MASK_U8 || ((uintptr_t)masks & 3) == 0, "cosy_instance_masks: int32 masks not 4-byte aligned");
    const long plane = (long)H * W;
    const bool wide = plane % 16 == 0 && aligned16(masks) && aligned16(out);
    const dim3 grid(cdiv(plane, (long)DET_THREADS * (wide ? 16 : 1)), N);
    if (dtype == COSY_MASK_U8) {
        const unsigned char* m = (const unsigned char*)masks;
        if (wide) hipLaunchKernelGGL((det_instance_masks_kernel<unsigned char, 16>), grid, dim3(DET_THREADS), 0, s, m, row_image, row_id, B, plane, out);
        else hipLaunchKernelGGL((det_instance_masks_kernel<unsigned char, 1>), grid, dim3(DET_THREADS), 0, s, m, row_image, row_id, B, plane, out);
    } else {
        const int* m = (const int*)masks;
        if (wide) hipLaunchKernelGGL((det_instance_masks_kernel<int, 16>), grid, dim3(DET_THREADS), 0, s, m, row_image, row_id, B, plane, out);
        else hipLaunchKernelGGL((det_instance_masks_kernel<int, 1>), grid, dim3(DET_THREADS), 0, s, m, row_image, row_id, B, plane, out);
    }
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

int cosy_box_iou_pairs(const float* a, const float* b, int N, float* iou, cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    COSY_REQUIRE(N >= 0, "cosy_box_iou_pairs: N=%d", N);
    if (N == 0) return COSY_OK;
    COSY_REQUIRE_PTR("cosy_box_iou_pairs", a); COSY_REQUIRE_PTR("cosy_box_iou_pairs", b); COSY_REQUIRE_PTR("cosy_box_iou_pairs", iou);
    if (aligned16(a) && aligned16(b)) hipLaunchKernelGGL(det_iou_pairs_kernel<true>, dim3(cdiv(N, DET_THREADS)), dim3(DET_THREADS), 0, s, a, b, N, iou);
    else hipLaunchKernelGGL(det_iou_pairs_kernel<false>, dim3(cdiv(N, DET_THREADS)), dim3(DET_THREADS), 0, s, a, b, N, iou);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

int cosy_box_iou_matrix(const float* a, const float* b, int N, int M, float* iou, cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    COSY_REQUIRE(N >= 0 && M >= 0, "cosy_box_iou_matrix: N=%d M=%d", N, M);
    COSY_REQUIRE(((long)N * M + DET_THREADS - 1) / DET_THREADS <= (long)INT_MAX, "cosy_box_iou_matrix: %d x %d pairs are too many for one call", N, M);
    if (N == 0 || M == 0) return COSY_OK;
    COSY_REQUIRE_PTR("cosy_box_iou_matrix", a); COSY_REQUIRE_PTR("cosy_box_iou_matrix", b); COSY_REQUIRE_PTR("cosy_box_iou_matrix", iou);
    const dim3 grid((unsigned)(((long)N * M + DET_THREADS - 1) / DET_THREADS));
    if (aligned16(a) && aligned16(b)) hipLaunchKernelGGL(det_iou_matrix_kernel<true>, grid, dim3(DET_THREADS), 0, s, a, b, N, M, iou);
    else hipLaunchKernelGGL(det_iou_matrix_kernel<false>, grid, dim3(DET_THREADS), 0, s, a, b, N, M, iou);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

}  // extern "C"
