// The order in which a launch of the backbone walks its jobs (included by net_device.h; plain C++ as well, so that a host program can check it).
// Every streaming kernel decodes its workgroup id as xcd = id & 7 (consecutive ids go round-robin over the 8 XCDs), jj = id >> 3 = the job
// index inside that XCD, sample-major.  A launch that READS a large activation walks jj in the opposite order to the launch that WROTE it
// (effnet.hip: plan_traversal), so that it starts with the bytes written last -- the ones the last-level cache may still hold.  `rev` is a
// run-time field of the kernel's argument struct: one scalar select per workgroup, the same kernel symbol for both orders.
// The XCD residue is kept: the jobs of a sample stay on their XCD, the waves of a workgroup stay neighbouring jobs of one sample, and the
// job-to-data mapping behind (xcd, jj) is untouched -- a reversed launch computes the same jobs, bit for bit, in another order.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define COSY_JOB_HD __host__ __device__ __forceinline__
#else
#define COSY_JOB_HD static inline
#endif

namespace cosy {

struct JobId { int xcd, jj; };

// grid: gridDim.x, a multiple of 8 (the launchers round the job count up to whole rounds of the 8 XCDs; the surplus workgroups decode a
// job beyond the count and return -- in a reversed launch they come first)
COSY_JOB_HD JobId job_decode(unsigned id, unsigned grid, int rev) {
    const int j = (int)(id >> 3);
    return JobId{(int)(id & 7), rev ? (int)(grid >> 3) - 1 - j : j};
}

// the kernels whose grid is a plain (sample, part) product of any size: the whole id is mirrored
COSY_JOB_HD int job_linear(unsigned id, unsigned grid, int rev) { return rev ? (int)(grid - 1 - id) : (int)id; }

}  // namespace cosy
