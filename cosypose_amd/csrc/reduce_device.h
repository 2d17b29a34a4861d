// Wave and workgroup reductions and the workgroup scan, each defined once.  Every order is fixed, so a result does not depend on
// which kernel asks: lanes by an xor tree with offsets 32..1, then waves 0..3 in sequence.  Every lane of the wave (every thread of
// the 256-thread workgroup) takes part; lanes without a value pass the neutral element.
#pragma once
#include <type_traits>

#include "cosy_common.h"

namespace cosy {

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
template <typename T>      // integers only: float has its own overloads below
__device__ __forceinline__ T wave_min(T v) {
    static_assert(std::is_integral<T>::value, "wave_min<T>: integers; float takes the fminf overload");
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}
template <typename T>
__device__ __forceinline__ T wave_max(T v) {
    static_assert(std::is_integral<T>::value, "wave_max<T>: integers; float takes the fmaxf overload");
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}
// float: fminf / fmaxf, a NaN loses against a number
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// sum over the 256 threads of a workgroup: wave_sum, then ((w0 + w1) + w2) + w3.  `scratch` = 4 values of LDS per reduced value.
// Returns the total in every thread.
template <typename T>
__device__ __forceinline__ T block_sum256(T v, T* scratch) {
    v = wave_sum(v);
    __syncthreads();   // scratch may still be read from the previous reduction
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((scratch[0] + scratch[1]) + scratch[2]) + scratch[3];
}

// inclusive scan (Hillis-Steele) of part[0..255] in LDS by the 256 threads of a workgroup; thread tid has written part[tid]
__device__ __forceinline__ void block_scan256(int* part) {
    const int tid = threadIdx.x;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const int v = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
}

}  // namespace cosy
