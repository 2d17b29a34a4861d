// BOP ground-truth annotations (what the BOP toolkit's calc_gt_masks.py and calc_gt_info.py write): per instance the pixel counts
// px_count_all / px_count_valid / px_count_visib, the boxes bbox_obj / bbox_visib, the visible masks and their composite per view.
// DESIGN.md section 19 holds the contract; tests/gt_ref.py restates it in numpy.
//
// An instance is drawn alone on a canvas of 3H x 3W whose centre third is the frame (K' = K with cx + W, cy + H), so the part of its
// silhouette outside the frame counts.  The drawing is not done here: cosy_bop_instance_boxes and cosy_bop_render_windows of
// kernels_bop.hip, called with K' and (3H, 3W), leave every instance's depth in a packed window the size of its own canvas box.
//
// cosy_gt_info.  Work = a flat list of (instance, strip of GT_STRIP window pixels) items (the queue of work_items.h).  Per pixel: the
// window depth; inside the frame the two distances of section 15 (image coordinates, the unshifted K) and the masks
//     mask = dist_gt > 0,   valid = mask and t > 0,   V = mask and (dist_gt - t <= delta or t == 0).
// Counts by ballots, boxes by wave min / max; an item ends in ONE integer atomic per count and per box side.  The composite is an
// atomicMax of id_in_segm into a zeroed int32 image (the highest id wins an overlap, as the sequential paint of
// cosypose/datasets/bop.py:151-153 does); the dense masks are byte stores of the window's part of the frame into zeroed images.
// Integer atomics only: the result does not depend on which workgroup takes which item.
//
// Built with contraction off (build.py FILE_FLAGS), as kernels_bop.hip: bop_device.h's distance has the same bits in both.
#include <limits.h>
#include "cosy_common.h"
#include "bop_device.h"
#include "work_items.h"

#pragma clang fp contract(off)

namespace cosy {

namespace {

constexpr int GT_STRIP = 256 * 8;            // window pixels per work item
constexpr int GT_GRID = 256 * 4;             // workgroups that draw items

struct GtTables {
    const int* inst_view;           // (N)
    const int* id_in_segm;          // (N)
    const int* boxes;               // (N,4) on the canvas
    const long long* win_offset;    // (N)
    const float* store;             // the windows
    long n_px;
    const float* depth_test;        // (n_views,H,W)
    const float* K;                 // (n_views,3,3), unshifted
    int N, n_views, H, W;
};

// the window of instance n on the 3H x 3W canvas; bw = 0 (no pixels at all) for an empty or dead box, a view outside the frame table or
// a window that does not lie in the store as a whole
__device__ __forceinline__ Window gt_window(const GtTables& t, int n) {
    Window w = window_of(t.boxes, t.win_offset, t.n_px, n, 3 * t.H, 3 * t.W);
    const int v = t.inst_view[n];
    if (w.bw && (v < 0 || v >= t.n_views || (long)w.bw * w.bh > w.room)) w.bw = 0;
    return w;
}

struct GtItems {
    GtTables t;
    __device__ int operator()(int n) const {
        const Window w = gt_window(t, n);
        return w.bw ? (int)(((long)w.bw * w.bh + GT_STRIP - 1) / GT_STRIP) : 0;
    }
};

// acc (N,11): px_count_all, px_count_valid, px_count_visib | x, y minima and maxima of {depth > 0} on the canvas | the same of V in the frame
__global__ __launch_bounds__(256) void gt_init_kernel(int N, int* __restrict__ acc) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N * 11) return;
    const int k = i % 11;
    acc[i] = k < 3 ? 0 : ((k - 3) & 2) ? INT_MIN : INT_MAX;       // 3 counts | min min max max | min min max max
}

__global__ __launch_bounds__(256) void gt_info_kernel(GtTables t, float delta, WorkPlan* __restrict__ plan, const int* __restrict__ start,
                                                      int* __restrict__ acc, int* __restrict__ composite, unsigned char* __restrict__ mask,
                                                      unsigned char* __restrict__ mask_visib) {
    __shared__ int red[4][11];
    const int tid = threadIdx.x, wave = tid >> 6;
    const int total = plan->total;
    const int H = t.H, W = t.W;
    for (;;) {
        const int item = next_item(plan);      // (a barrier: red of the previous item is no longer read)
        if (item >= total) return;
        const int n = row_of_item(start, t.N, item);
        const Window w = gt_window(t, n);
        if (w.bw == 0) continue;               // (an instance with items has a window; block-uniform)
        const int strip = item - start[n];
        const long npx = (long)w.bw * w.bh;    // <= w.room: gt_window admits no other window
        const int view = t.inst_view[n], id = t.id_in_segm[n];
        const float* Kv = t.K + (size_t)view * 9;
        const float fx = Kv[0], fy = Kv[4], cx = Kv[2], cy = Kv[5];
        const size_t frame_at = (size_t)view * H * W, inst_at = (size_t)n * H * W;
        int n_all = 0, n_valid = 0, n_vis = 0;
        int ox0 = INT_MAX, oy0 = INT_MAX, ox1 = INT_MIN, oy1 = INT_MIN, vx0 = INT_MAX, vy0 = INT_MAX, vx1 = INT_MIN, vy1 = INT_MIN;
        for (int j = 0; j < GT_STRIP / 256; ++j) {
            const long i = (long)strip * GT_STRIP + j * 256 + tid;
            bool all = false, valid = false, vis = false;
            if (i < npx) {
                const int wy = (int)(i / w.bw), xc = w.x0 + (int)(i - (long)wy * w.bw), yc = w.y0 + wy;      // on the canvas
                const float z = t.store[w.off + i];
                all = z > 0.f;
                if (all) { ox0 = min(ox0, xc); oy0 = min(oy0, yc); ox1 = max(ox1, xc); oy1 = max(oy1, yc); }
                const int x = xc - W, y = yc - H;                                                          // in the frame's coordinates
                if (x >= 0 && x < W && y >= 0 && y < H) {
                    const size_t px = (size_t)y * W + x;
                    const float xk = (float)x - cx, yk = (float)y - cy;
                    const float dg = depth_to_dist(z, xk, yk, fx, fy);
                    const float dt = depth_to_dist(t.depth_test[frame_at + px], xk, yk, fx, fy);
                    const bool m = dg > 0.f;
                    valid = m && dt > 0.f;
                    vis = m && (dg - dt <= delta || dt == 0.f);
                    if (vis) {
                        vx0 = min(vx0, x); vy0 = min(vy0, y); vx1 = max(vx1, x); vy1 = max(vy1, y);
                        atomicMax(composite + frame_at + px, id);
                    }
                    if (mask) mask[inst_at + px] = m ? 1 : 0;
                    if (mask_visib) mask_visib[inst_at + px] = vis ? 1 : 0;
                }
            }
            n_all += __popcll(__ballot(all));
            n_valid += __popcll(__ballot(valid));
            n_vis += __popcll(__ballot(vis));
        }
        ox0 = wave_min(ox0); oy0 = wave_min(oy0); ox1 = wave_max(ox1); oy1 = wave_max(oy1);
        vx0 = wave_min(vx0); vy0 = wave_min(vy0); vx1 = wave_max(vx1); vy1 = wave_max(vy1);
        if ((tid & 63) == 0) {
            int* r = red[wave];
            r[0] = n_all; r[1] = n_valid; r[2] = n_vis;
            r[3] = ox0; r[4] = oy0; r[5] = ox1; r[6] = oy1; r[7] = vx0; r[8] = vy0; r[9] = vx1; r[10] = vy1;
        }
        __syncthreads();
        if (tid < 11) {
            const int a = red[0][tid], b = red[1][tid], c = red[2][tid], d = red[3][tid];
            int* out = acc + (size_t)n * 11 + tid;
            if (tid < 3) {
                const int sum = (a + b) + (c + d);
                if (sum) atomicAdd(out, sum);
            } else if ((tid - 3) & 2) {
                const int hi = max(max(a, b), max(c, d));
                if (hi != INT_MIN) atomicMax(out, hi);
            } else {
                const int lo = min(min(a, b), min(c, d));
                if (lo != INT_MAX) atomicMin(out, lo);
            }
        }
    }
}

// counts (N,3) and the two boxes in the toolkit's x, y, w, h (w = max - min): bbox_obj in the frame's coordinates (it may be negative or
// reach past the frame), both -1 when nothing of the instance is visible
__global__ __launch_bounds__(256) void gt_final_kernel(int N, int H, int W, const int* __restrict__ acc, int* __restrict__ counts,
                                                       int* __restrict__ bbox_obj, int* __restrict__ bbox_visib) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const int* a = acc + (size_t)n * 11;
    counts[n * 3] = a[0]; counts[n * 3 + 1] = a[1]; counts[n * 3 + 2] = a[2];
    const bool seen = a[2] > 0;
    bbox_obj[n * 4] = seen ? a[3] - W : -1;
    bbox_obj[n * 4 + 1] = seen ? a[4] - H : -1;
    bbox_obj[n * 4 + 2] = seen ? a[5] - a[3] : -1;
    bbox_obj[n * 4 + 3] = seen ? a[6] - a[4] : -1;
    bbox_visib[n * 4] = seen ? a[7] : -1;
    bbox_visib[n * 4 + 1] = seen ? a[8] : -1;
    bbox_visib[n * 4 + 2] = seen ? a[9] - a[7] : -1;
    bbox_visib[n * 4 + 3] = seen ? a[10] - a[8] : -1;
}

__global__ __launch_bounds__(256) void gt_narrow_kernel(const int* __restrict__ composite, long n, unsigned char* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (unsigned char)min(max(composite[i], 0), 255);
}

}  // namespace

}  // namespace cosy

using namespace cosy;

extern "C" {

size_t cosy_gt_info_workspace_bytes(int N) { return N <= 0 ? 0 : work_plan_bytes(N) + ((size_t)N * 11 * sizeof(int) + 15) / 16 * 16; }

int cosy_gt_info(const int* inst_view, const int* id_in_segm, const int* boxes, const long long* win_offset, const float* windows,
                 long long n_pixels, const float* depth_test, const float* K, float delta, int N, int n_views, int H, int W, int* counts,
                 int* bbox_obj, int* bbox_visib, int* composite, unsigned char* mask, unsigned char* mask_visib, void* workspace,
                 size_t workspace_bytes, cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    COSY_REQUIRE(N >= 0 && n_views > 0 && H > 0 && W > 0 && n_pixels >= 0, "cosy_gt_info: N=%d n_views=%d H=%d W=%d n_pixels=%lld", N, n_views, H, W,
                 n_pixels);
    COSY_REQUIRE(9L * H * W < (1L << 31), "cosy_gt_info: the canvas of 3 H x 3 W = %ld pixels exceeds 2^31 (H=%d W=%d)", 9L * H * W, H, W);
    COSY_REQUIRE((long)N * cdiv(9L * H * W, GT_STRIP) < (1L << 31), "cosy_gt_info: N=%d x %d strips of H=%d W=%d exceed 2^31 items", N,
                 cdiv(9L * H * W, GT_STRIP), H, W);
    if (N == 0) return COSY_OK;
    COSY_REQUIRE_PTR("cosy_gt_info", inst_view); COSY_REQUIRE_PTR("cosy_gt_info", id_in_segm);
    COSY_REQUIRE_PTR("cosy_gt_info", boxes); COSY_REQUIRE_PTR("cosy_gt_info", win_offset);
    COSY_REQUIRE_PTR("cosy_gt_info", depth_test); COSY_REQUIRE_PTR("cosy_gt_info", K);
    COSY_REQUIRE_PTR("cosy_gt_info", counts); COSY_REQUIRE_PTR("cosy_gt_info", bbox_obj);
    COSY_REQUIRE_PTR("cosy_gt_info", bbox_visib); COSY_REQUIRE_PTR("cosy_gt_info", composite);
    COSY_REQUIRE_PTR("cosy_gt_info", workspace);
    COSY_REQUIRE(n_pixels == 0 || windows, "cosy_gt_info: null windows with n_pixels=%lld", n_pixels);
    COSY_REQUIRE(workspace_bytes >= cosy_gt_info_workspace_bytes(N), "cosy_gt_info: workspace_bytes=%zu < %zu", workspace_bytes,
                 cosy_gt_info_workspace_bytes(N));
    COSY_REQUIRE(((uintptr_t)workspace & 15) == 0, "cosy_gt_info: workspace not 16-byte aligned");
    WorkPlan* plan = (WorkPlan*)workspace;
    int* start = (int*)(plan + 1);
    int* acc = (int*)((char*)workspace + work_plan_bytes(N));
    const GtTables t{inst_view, id_in_segm, boxes, win_offset, windows, (long)n_pixels, depth_test, K, N, n_views, H, W};
    hipLaunchKernelGGL(gt_init_kernel, dim3(cdiv((long)N * 11, 256)), dim3(256), 0, s, N, acc);
    COSY_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(work_plan_kernel<GtItems>, dim3(1), dim3(256), 0, s, GtItems{t}, N, plan, start);
    COSY_CHECK_HIP(hipGetLastError());
    const long max_items = (long)N * cdiv(9L * H * W, GT_STRIP);
    hipLaunchKernelGGL(gt_info_kernel, dim3((unsigned)(max_items < GT_GRID ? max_items : GT_GRID)), dim3(256), 0, s, t, delta, plan, (const int*)start,
                       acc, composite, mask, mask_visib);
    COSY_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(gt_final_kernel, dim3(cdiv(N, 256)), dim3(256), 0, s, N, H, W, (const int*)acc, counts, bbox_obj, bbox_visib);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

int cosy_gt_composite_u8(const int* composite, long long n, unsigned char* out, cosy_stream_t stream) {
    COSY_REQUIRE(n >= 0, "cosy_gt_composite_u8: n=%lld", n);
    COSY_REQUIRE((n + 255) / 256 < (1LL << 31), "cosy_gt_composite_u8: n=%lld exceeds 2^31 blocks", n);
    if (n == 0) return COSY_OK;
    COSY_REQUIRE_PTR("cosy_gt_composite_u8", composite); COSY_REQUIRE_PTR("cosy_gt_composite_u8", out);
    hipLaunchKernelGGL(gt_narrow_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, composite, (long)n, out);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

}  // extern "C"
