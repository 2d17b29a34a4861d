// The work-item queue of kernels_eval.hip and kernels_bop.hip.  Work = a flat list of items, items(b) of them for row b of a batch;
// a one-workgroup plan kernel turns the counts into start[B + 1] by a prefix sum, workgroups then draw item numbers from an integer
// counter until it passes the total.  The batch is no grid dimension and rows of mixed sizes keep every CU busy.  Which workgroup
// takes an item must have no effect on the result.  All integer arithmetic.
#pragma once
#include "reduce_device.h"

namespace cosy {

struct WorkPlan {     // head of a workspace, followed by start[B + 1]
    int total;        // number of items
    int next;         // the item counter
};

static inline size_t work_plan_bytes(int B) { return (sizeof(WorkPlan) + ((size_t)B + 1) * sizeof(int) + 15) / 16 * 16; }

// start[b] = number of items before row b (start[B] = total), by one workgroup: every thread sums a contiguous run of rows, the 256
// run totals are scanned in LDS, every thread writes its run.  Also resets the item counter.
template <class Items>
__global__ __launch_bounds__(256) void work_plan_kernel(Items items, int B, WorkPlan* __restrict__ plan, int* __restrict__ start) {
    __shared__ int part[256];
    const int tid = threadIdx.x, run = (B + 255) / 256;
    const int b0 = min(B, tid * run), b1 = min(B, b0 + run);
    int sum = 0;
    for (int b = b0; b < b1; ++b) sum += items(b);
    part[tid] = sum;
    block_scan256(part);
    int at = part[tid] - sum;
    for (int b = b0; b < b1; ++b) {
        start[b] = at;
        at += items(b);
    }
    if (tid == 255) { start[B] = part[255]; plan->total = part[255]; plan->next = 0; }
}

// the row of an item: the last b with start[b] <= item (rows without items share their successor's start)
__device__ __forceinline__ int row_of_item(const int* __restrict__ start, int B, int item) {
    int lo = 0, hi = B;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (start[mid] <= item) lo = mid; else hi = mid;
    }
    return lo;
}

// Head of a workgroup's item loop: the next item for every thread, or a number >= plan->total when the list is used up.  The leading
// barrier also ends the previous item: what that item kept in LDS is no longer read.
__device__ __forceinline__ int next_item(WorkPlan* __restrict__ plan) {
    __shared__ int item_s;
    __syncthreads();
    if (threadIdx.x == 0) item_s = atomicAdd(&plan->next, 1);
    __syncthreads();
    return item_s;
}

}  // namespace cosy
