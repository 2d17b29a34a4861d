// 4x4 pose helpers shared by the float32 distance kernels (kernels_dist.hip, kernels_ransac.hip).  Fixed operation order and NO
// contraction (the pragma below holds for the rest of the translation unit, which is what both files want): every multiply and add
// rounds on its own, so a value equals the CPU restatement's bit for bit and does not depend on the kernel that computes it.
#pragma once
#include "cosy_common.h"

#pragma clang fp contract(off)

namespace cosy {

__device__ __forceinline__ void mat4_mul(const float* A, const float* Bm, float* C) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) acc += A[i * 4 + k] * Bm[k * 4 + j];
            C[i * 4 + j] = acc;
        }
}
// transform_pts (lib3d/transform_ops.py:7-21): R p + t
__device__ __forceinline__ void xform_pt(const float* T, float x, float y, float z, float* q) {
#pragma unroll
    for (int i = 0; i < 3; ++i) q[i] = ((T[i * 4 + 0] * x + T[i * 4 + 1] * y) + T[i * 4 + 2] * z) + T[i * 4 + 3];
}

}  // namespace cosy
