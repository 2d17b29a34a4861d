// Pose evaluation errors: ADD / ADD-S / ADD(-S) reduced to the 8 numbers per tentative (prediction, ground truth) pair that
// PoseErrorMeter.compute_errors keeps (cosypose/evaluation/meters/pose_meters.py:53-92): mean norm and mean |x|,|y|,|z| of the
// per-point vectors, |t_pred - t_gt| and its norm.  The (B,P,3) vectors of cosy_dists_add never reach memory.
//
// The per-point vectors are the bits of dists_add_kernel (kernels_dist.hip): xform_pt of dist_device.h, the squared distance as
// (dx*dx + dy*dy) + dz*dz, contraction off, strict < with the first minimum winning, the first predicted point taken
// unconditionally (a NaN there stays).  No |g|^2 + |q|^2 - 2 g.q form.
//
// Work = a flat list of (candidate, tile of EVAL_TILE ground-truth points) items, found from a prefix sum of the candidates' tile
// counts (the queue of work_items.h); workgroups draw items from an integer counter, so a batch of mixed mesh sizes keeps every CU
// busy and B is not bounded by a grid dimension.  Which workgroup computes an item has no effect on the result: every item writes its own
// 4 float64 partial sums, summed within the workgroup in a fixed order (lane tree, then waves 0..3), and eval_final_kernel adds a
// candidate's tiles in tile order.  No floating-point atomics; a candidate's result depends on its own pose and points only.
//
// ADD-S inner loop: the predicted points of a chunk sit in LDS as padded float4, so that every point is one 16-byte-aligned read
// of the same address in all lanes (a broadcast; hipcc emits ds_read_b96, the pad is never loaded); every thread holds EVAL_G
// ground-truth points in registers, so one LDS read feeds EVAL_G distance evaluations of 11 VALU instructions each (3 sub, 3 mul,
// 2 add, compare, 2 selects: the running minimum and the INDEX of its point -- the vector is recomputed from the index once, after
// the scan).
#include "cosy_common.h"
#include "dist_device.h"
#include "work_items.h"

#pragma clang fp contract(off)

namespace cosy {

namespace {

constexpr int EVAL_G = 4;                    // ground-truth points per thread
constexpr int EVAL_TILE = 256 * EVAL_G;      // ground-truth points per work item
constexpr int EVAL_CHUNK = 2048;             // predicted points staged in LDS per pass (32 KB as float4)
constexpr int EVAL_GRID = 256 * 4;           // workgroups that draw items: 4 per CU fit beside their 32 KB of LDS

__device__ __forceinline__ int eval_points_of(const int* __restrict__ obj_id, const int* __restrict__ n_points, int b, int n_obj, int n_max) {
    const int o = obj_id[b];
    if (o < 0 || o >= n_obj) return 0;                 // a row outside the table contributes nothing: its errors come out NaN
    const int n = n_points[o];
    return n < 0 ? 0 : (n > n_max ? n_max : n);
}

struct EvalItems {    // tiles of a candidate
    const int* obj_id;
    const int* n_points;
    int n_obj, n_max;
    __device__ int operator()(int b) const { return (eval_points_of(obj_id, n_points, b, n_obj, n_max) + EVAL_TILE - 1) / EVAL_TILE; }
};

__global__ __launch_bounds__(256) void eval_tiles_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                         const int* __restrict__ obj_id, const int* __restrict__ mode,
                                                         const float* __restrict__ pts, const int* __restrict__ n_points, int B, int n_obj,
                                                         int n_max, WorkPlan* __restrict__ plan, const int* __restrict__ start,
                                                         double* __restrict__ partial) {
    __shared__ float4 pp[EVAL_CHUNK];
    __shared__ double red[16];
    const int tid = threadIdx.x;
    const int total = plan->total;
    for (;;) {
        const int item = next_item(plan);      // (a barrier: pp and red of the previous item are no longer read)
        if (item >= total) return;
        const int b = row_of_item(start, B, item), tile = item - start[b];
        const int P = eval_points_of(obj_id, n_points, b, n_obj, n_max);
        const float* p = pts + (size_t)obj_id[b] * n_max * 3;      // P > 0 here, so obj_id[b] is a row of the table
        const bool symmetric = mode[b] != 0;
        float tp[16], tg[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) { tp[k] = pred[(size_t)b * 16 + k]; tg[k] = gt[(size_t)b * 16 + k]; }
        float g[EVAL_G][3], r[EVAL_G][3];
        int gi[EVAL_G];
#pragma unroll
        for (int k = 0; k < EVAL_G; ++k) {
            gi[k] = tile * EVAL_TILE + k * 256 + tid;
            g[k][0] = g[k][1] = g[k][2] = 0.f;
            if (gi[k] < P) xform_pt(tg, p[gi[k] * 3], p[gi[k] * 3 + 1], p[gi[k] * 3 + 2], g[k]);
        }
        if (!symmetric) {
#pragma unroll
            for (int k = 0; k < EVAL_G; ++k) {
                float q[3] = {0.f, 0.f, 0.f};
                if (gi[k] < P) xform_pt(tp, p[gi[k] * 3], p[gi[k] * 3 + 1], p[gi[k] * 3 + 2], q);
                r[k][0] = g[k][0] - q[0]; r[k][1] = g[k][1] - q[1]; r[k][2] = g[k][2] - q[2];
            }
        } else {
            float best[EVAL_G];
            int arg[EVAL_G];
            for (int j0 = 0; j0 < P; j0 += EVAL_CHUNK) {
                const int nj = min(EVAL_CHUNK, P - j0);
                __syncthreads();
                for (int j = tid; j < nj; j += 256) {
                    float q[3];
                    xform_pt(tp, p[(j0 + j) * 3], p[(j0 + j) * 3 + 1], p[(j0 + j) * 3 + 2], q);
                    pp[j] = make_float4(q[0], q[1], q[2], 0.f);
                }
                __syncthreads();
                if (j0 == 0) {     // the first predicted point is taken whatever its distance (a NaN stays: nothing is < NaN)
                    const float4 q = pp[0];
#pragma unroll
                    for (int k = 0; k < EVAL_G; ++k) {
                        const float dx = g[k][0] - q.x, dy = g[k][1] - q.y, dz = g[k][2] - q.z;
                        best[k] = (dx * dx + dy * dy) + dz * dz;
                        arg[k] = 0;
                    }
                }
#pragma unroll 4
                for (int j = 0; j < nj; ++j) {
                    const float4 q = pp[j];
#pragma unroll
                    for (int k = 0; k < EVAL_G; ++k) {
                        const float dx = g[k][0] - q.x, dy = g[k][1] - q.y, dz = g[k][2] - q.z;
                        const float sq = (dx * dx + dy * dy) + dz * dz;
                        const bool take = sq < best[k];
                        best[k] = take ? sq : best[k];
                        arg[k] = take ? j0 + j : arg[k];
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < EVAL_G; ++k) {
                float q[3];
                xform_pt(tp, p[arg[k] * 3], p[arg[k] * 3 + 1], p[arg[k] * 3 + 2], q);      // arg < P: the bits that were in LDS
                r[k][0] = g[k][0] - q[0]; r[k][1] = g[k][1] - q[1]; r[k][2] = g[k][2] - q[2];
            }
        }
        double s[4] = {0., 0., 0., 0.};
#pragma unroll
        for (int k = 0; k < EVAL_G; ++k)
            if (gi[k] < P) {
                s[0] += (double)sqrtf((r[k][0] * r[k][0] + r[k][1] * r[k][1]) + r[k][2] * r[k][2]);
                s[1] += (double)fabsf(r[k][0]); s[2] += (double)fabsf(r[k][1]); s[3] += (double)fabsf(r[k][2]);
            }
        // fixed-order float64 sums over the workgroup, the order of block_sum256 without its leading barrier: the four sums use
        // disjoint parts of red, and the barrier of next_item protects its reuse
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            s[c] = wave_sum(s[c]);
            if ((tid & 63) == 0) red[4 * c + (tid >> 6)] = s[c];
        }
        __syncthreads();
        if (tid < 4) partial[(size_t)item * 4 + tid] = ((red[4 * tid] + red[4 * tid + 1]) + red[4 * tid + 2]) + red[4 * tid + 3];
    }
}

// a candidate's tiles summed in tile order, the means, and the translation errors
__global__ __launch_bounds__(256) void eval_final_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                         const int* __restrict__ obj_id, const int* __restrict__ n_points, int B, int n_obj,
                                                         int n_max, const int* __restrict__ start, const double* __restrict__ partial,
                                                         float* __restrict__ errors) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const int P = eval_points_of(obj_id, n_points, b, n_obj, n_max);
    double s[4] = {0., 0., 0., 0.};
    for (int it = start[b]; it < start[b + 1]; ++it)
#pragma unroll
        for (int c = 0; c < 4; ++c) s[c] += partial[(size_t)it * 4 + c];
    float* e = errors + (size_t)b * 8;
#pragma unroll
    for (int c = 0; c < 4; ++c) e[c] = (float)(s[c] / (double)P);      // P = 0: 0 / 0 = NaN, the mean of nothing
    const float dx = pred[(size_t)b * 16 + 3] - gt[(size_t)b * 16 + 3], dy = pred[(size_t)b * 16 + 7] - gt[(size_t)b * 16 + 7],
                dz = pred[(size_t)b * 16 + 11] - gt[(size_t)b * 16 + 11];
    e[4] = fabsf(dx); e[5] = fabsf(dy); e[6] = fabsf(dz);
    e[7] = sqrtf((dx * dx + dy * dy) + dz * dz);
}

}  // namespace

}  // namespace cosy

using namespace cosy;

extern "C" {

size_t cosy_pose_errors_workspace_bytes(int B, int n_max) {
    if (B <= 0 || n_max <= 0) return 0;
    return work_plan_bytes(B) + (size_t)B * cdiv(n_max, EVAL_TILE) * 4 * sizeof(double);
}

int cosy_pose_errors(const float* TXO_pred, const float* TXO_gt, const int* obj_id, const int* mode, const float* pts_table,
                     const int* n_points, int B, int n_obj, int n_max, float* errors, void* workspace, size_t workspace_bytes,
                     cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    COSY_REQUIRE(B >= 0 && n_obj > 0 && n_max > 0, "cosy_pose_errors: B=%d n_obj=%d n_max=%d", B, n_obj, n_max);
    COSY_REQUIRE((long)B * cdiv(n_max, EVAL_TILE) < (1L << 31), "cosy_pose_errors: B=%d x %d tiles of n_max=%d exceed 2^31 items", B,
                 cdiv(n_max, EVAL_TILE), n_max);
    if (B == 0) return COSY_OK;
    COSY_REQUIRE_PTR("cosy_pose_errors", TXO_pred); COSY_REQUIRE_PTR("cosy_pose_errors", TXO_gt);
    COSY_REQUIRE_PTR("cosy_pose_errors", obj_id); COSY_REQUIRE_PTR("cosy_pose_errors", mode);
    COSY_REQUIRE_PTR("cosy_pose_errors", pts_table); COSY_REQUIRE_PTR("cosy_pose_errors", n_points);
    COSY_REQUIRE_PTR("cosy_pose_errors", errors); COSY_REQUIRE_PTR("cosy_pose_errors", workspace);
    COSY_REQUIRE(workspace_bytes >= cosy_pose_errors_workspace_bytes(B, n_max), "cosy_pose_errors: workspace_bytes=%zu < %zu",
                 workspace_bytes, cosy_pose_errors_workspace_bytes(B, n_max));
    COSY_REQUIRE(((uintptr_t)workspace & 15) == 0, "cosy_pose_errors: workspace not 16-byte aligned");
    WorkPlan* plan = (WorkPlan*)workspace;
    int* start = (int*)(plan + 1);
    double* partial = (double*)((char*)workspace + work_plan_bytes(B));
    hipLaunchKernelGGL(work_plan_kernel<EvalItems>, dim3(1), dim3(256), 0, s, EvalItems{obj_id, n_points, n_obj, n_max}, B, plan, start);
    COSY_CHECK_HIP(hipGetLastError());
    const long max_items = (long)B * cdiv(n_max, EVAL_TILE);
    hipLaunchKernelGGL(eval_tiles_kernel, dim3((unsigned)(max_items < EVAL_GRID ? max_items : EVAL_GRID)), dim3(256), 0, s, TXO_pred, TXO_gt,
                       obj_id, mode, pts_table, n_points, B, n_obj, n_max, plan, start, partial);
    COSY_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(eval_final_kernel, dim3(cdiv(B, 256)), dim3(256), 0, s, TXO_pred, TXO_gt, obj_id, n_points, B, n_obj, n_max, start,
                       partial, errors);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

}  // extern "C"
