// What kernels_frames.hip and kernels_detin.hip (section 25) must do alike, to the last bit, one definition each.  Both
// resize through the host-made tables of section 18: per axis and output index a 16-byte tap entry (i0, i1, bits of l0, bits of l1) and a
// nearest source index, at offsets (in ints) that a descriptor names.  Here: the rules those offsets must meet before anything is read
// through them, the tap entry's load, the two-tap bilinear sample, the nearest gather and the packed byte store.  The includers are compiled
// with -ffp-contract=off (build.FILE_FLAGS covers this header); fused operations are spelled fmaf, lone products __fmul_rn.
#pragma once
#include "cosy_common.h"

namespace cosy {

constexpr int IMG_PX = 4;                                    // horizontally adjacent outputs of one row that a thread owns

__host__ __device__ __forceinline__ int clamp_index(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }

// `n` ints at offset `b` lie inside the `n_tables` ints of the tables
__host__ __device__ __forceinline__ bool table_inside(long b, long n, long n_tables) { return b >= 0 && b + n <= n_tables; }
// the nearest table of an axis of `n` outputs: one int each
__host__ __device__ __forceinline__ bool nearest_table_ok(long b, long n, long n_tables) { return table_inside(b, n, n_tables); }
// the tap table of an axis of `n` outputs: four ints each, read as one 16-byte entry, so `b` is a multiple of 4 (the tables themselves are 16-byte aligned)
__host__ __device__ __forceinline__ bool tap_table_aligned(long b) { return (b & 3) == 0; }
__host__ __device__ __forceinline__ bool tap_table_ok(long b, long n, long n_tables) { return table_inside(b, 4 * n, n_tables) && tap_table_aligned(b); }

// one output index of one axis: the two source indices, clamped into the line, and their float32 weights
struct AxisTap { int i0, i1; float l0, l1; };

// entry `i` of the tap table at offset `base` (tap_table_ok) of an axis with `n_in` sources: one 16-byte load
__device__ __forceinline__ AxisTap load_tap(const int* __restrict__ tables, int base, int i, int n_in) {
    const int4 t = *reinterpret_cast<const int4*>(tables + base + 4 * (size_t)i);
    return {clamp_index(t.x, n_in - 1), clamp_index(t.y, n_in - 1), __int_as_float(t.z), __int_as_float(t.w)};
}

// the bilinear sample of DESIGN.md section 18 from its four looked-up values p[row tap][column tap]: three fused multiply-adds and three
// lone products, in this order and no other
__device__ __forceinline__ float two_tap(const AxisTap& tx, const AxisTap& ty, float p00, float p01, float p10, float p11) {
    const float lx0 = tx.l0, lx1 = tx.l1, ly0 = ty.l0, ly1 = ty.l1;
    const float top = fmaf(lx0, p00, __fmul_rn(lx1, p01));
    const float bot = fmaf(lx0, p10, __fmul_rn(lx1, p11));
    return fmaf(ly0, top, __fmul_rn(ly1, bot));
}

// px[j] = row[tables[at + j]], clamped into the n_in bytes of `row`, for the first n_valid of IMG_PX adjacent outputs of a nearest table
__device__ __forceinline__ void gather_nearest(const unsigned char* __restrict__ row, const int* __restrict__ tables, int at, int n_in, int n_valid,
                                               unsigned* px) {
#pragma unroll
    for (int j = 0; j < IMG_PX; ++j)
        if (j < n_valid) px[j] = row[clamp_index(tables[at + j], n_in - 1)];
}

// the valid bytes of px[] to p: one dword where all four are there and p is 4-byte aligned
__device__ __forceinline__ void store_px4(unsigned char* p, const unsigned* px, int n_valid) {
    if (n_valid == IMG_PX && ((uintptr_t)p & 3) == 0) {
        *reinterpret_cast<unsigned*>(p) = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
        return;
    }
#pragma unroll
    for (int j = 0; j < IMG_PX; ++j)
        if (j < n_valid) p[j] = (unsigned char)px[j];
}

}  // namespace cosy
