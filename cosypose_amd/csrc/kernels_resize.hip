// Pillow 12's Image.resize of 8-bit images, bilinear and bicubic, byte for byte (BackgroundAugmentation.__call__ of the reference resizes a
// background of any size to the frame before the paste: cosypose/datasets/augmentations.py:120-124).  DESIGN.md section 17 states the
// arithmetic; tests/resize_ref.py is its numpy twin.
//
// Host: cosy_resize_coeffs computes, in double and with one rounding per operation, the bounds (first tap, number of taps) and the 2^-22
// integer coefficients of every output index of one axis.  The file is compiled with contraction off (the pragma below and
// -ffp-contract=off in build.FILE_FLAGS): a fused multiply-add in the filter polynomial gives other coefficients.
// Device: integer arithmetic only, two launches over a batch of images of ANY sizes (a per-image descriptor names the source and, by offsets
// into one int32 table, the bounds and coefficients of its two axes; cosypose_amd/_tables.py packs both):
//   resize_rows_kernel   the horizontal pass, items -> workspace as BYTES (or -> out for an image that has no vertical pass)
//   resize_cols_kernel   the vertical pass, workspace -> out (or items -> out where there was no horizontal pass; an image already at
//                        (H, W) is copied through the same loop with one tap of weight 2^22)
// A thread owns RS_PX consecutive output bytes of one row and walks the C planes; a wave owns one row, so the bounds and coefficients of the
// vertical pass are wave-uniform.  Every workgroup takes its image's branches uniformly.  Nothing is staged in LDS: the taps of neighbouring
// outputs overlap and are served by the vector L1 / L2.  No shape is refused for its scale factor: a pass reads as many taps as its axis has.
#include "cosy_common.h"

#include <math.h>
#include <vector>

#pragma clang fp contract(off)

namespace cosy {
namespace {

constexpr int RS_THREADS = 256, RS_LANES = 64, RS_ROWS = RS_THREADS / RS_LANES, RS_PX = 4, RS_TILE_W = RS_LANES * RS_PX;
constexpr int RS_BITS = 22;                                  // Pillow's PRECISION_BITS = 32 - 8 - 2
constexpr int RS_MAX_AXIS = 1 << 24;                         // the longest axis cosy_resize_coeffs serves: ksize stays far inside int

double bilinear_filter(double x) {
    if (x < 0.0) x = -x;
    if (x < 1.0) return 1.0 - x;
    return 0.0;
}

double bicubic_filter(double x) {                            // Keys, a = -0.5
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

bool filter_support(int filter, double& support) {
    if (filter == COSY_RESIZE_BILINEAR) { support = 1.0; return true; }
    if (filter == COSY_RESIZE_BICUBIC) { support = 2.0; return true; }
    return false;
}

struct ResizeItem {
    const unsigned char* src;
    int h, w, hks, vks;
    const int *hb, *hk, *vb, *vk;
    bool ok;
};

__device__ __forceinline__ bool axis_ok(int b, int k, int ks, int out, long n_tables) {
    return b >= 0 && k >= 0 && (long)b + 2L * out <= n_tables && (long)k + (long)out * ks <= n_tables;
}

// An item the kernels cannot serve is skipped by BOTH launches: its image of `out` stays untouched and nothing is read through it.
__device__ __forceinline__ ResizeItem resize_load(const cosy_resize_item_t* __restrict__ items, int i, int H, int W, int max_h,
                                                  const int* __restrict__ tables, long n_tables) {
    const cosy_resize_item_t it = items[i];
    ResizeItem r;
    r.src = it.src; r.h = it.h; r.w = it.w; r.hks = it.hks; r.vks = it.vks;
    bool ok = it.src != nullptr && it.h >= 1 && it.w >= 1 && it.h <= max_h && it.hks >= 0 && it.vks >= 0;
    ok = ok && (it.hks ? axis_ok(it.hb, it.hk, it.hks, W, n_tables) : it.w == W);
    ok = ok && (it.vks ? axis_ok(it.vb, it.vk, it.vks, H, n_tables) : it.h == H);
    r.ok = ok;
    r.hb = tables + (ok ? it.hb : 0); r.hk = tables + (ok ? it.hk : 0);
    r.vb = tables + (ok ? it.vb : 0); r.vk = tables + (ok ? it.vk : 0);
    return r;
}

// first tap `a` and number of taps `n` of one output index, as the table gives them: served only when every tap lies inside the line
__device__ __forceinline__ bool bounds_ok(int a, int n, int ks, int in) { return a >= 0 && n >= 0 && n <= ks && a <= in - n; }

__device__ __forceinline__ unsigned clip8(int acc) {
    const int v = acc >> RS_BITS;                            // arithmetic shift: bicubic's negative lobes reach below zero
    return v < 0 ? 0u : v > 255 ? 255u : (unsigned)v;
}

// the valid bytes of px[] to p: one dword where all four are there and p is 4-byte aligned
__device__ __forceinline__ void store_px(unsigned char* p, const unsigned* px, const bool* valid, bool all) {
    if (all && ((uintptr_t)p & 3) == 0) {
        *reinterpret_cast<unsigned*>(p) = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
        return;
    }
#pragma unroll
    for (int j = 0; j < RS_PX; ++j)
        if (valid[j]) p[j] = (unsigned char)px[j];
}

__global__ __launch_bounds__(RS_THREADS) void resize_rows_kernel(const cosy_resize_item_t* __restrict__ items, int C, int H, int W, int max_h,
                                                                 const int* __restrict__ tables, long n_tables, unsigned char* __restrict__ out,
                                                                 unsigned char* __restrict__ ws) {
    const int i = blockIdx.z;
    const ResizeItem it = resize_load(items, i, H, W, max_h, tables, n_tables);
    if (!it.ok || it.hks == 0) return;
    const int y = blockIdx.y * RS_ROWS + __builtin_amdgcn_readfirstlane(threadIdx.x / RS_LANES);
    const int x0 = (blockIdx.x * RS_LANES + (threadIdx.x % RS_LANES)) * RS_PX;
    if (y >= it.h || x0 >= W) return;
    // without a vertical pass h == H and the rows are the result; else they go to this image's slot of the workspace, C planes of h x W
    unsigned char* dst = it.vks ? ws + (size_t)i * C * max_h * W : out + (size_t)i * C * H * W;
    int xmin[RS_PX], xmax[RS_PX];
    bool valid[RS_PX], all = true;
#pragma unroll
    for (int j = 0; j < RS_PX; ++j) {
        valid[j] = false;
        xmin[j] = xmax[j] = 0;
        if (x0 + j < W) {
            const int a = it.hb[2 * (x0 + j)], n = it.hb[2 * (x0 + j) + 1];
            if (bounds_ok(a, n, it.hks, it.w)) { valid[j] = true; xmin[j] = a; xmax[j] = n; }
        }
        all = all && valid[j];
    }
    for (int c = 0; c < C; ++c) {
        const unsigned char* row = it.src + ((size_t)c * it.h + y) * it.w;
        unsigned px[RS_PX];
#pragma unroll
        for (int j = 0; j < RS_PX; ++j) {
            const int* kk = it.hk + (size_t)(x0 + j) * it.hks;
            const unsigned char* p = row + xmin[j];
            int acc = 1 << (RS_BITS - 1);
            for (int t = 0; t < xmax[j]; ++t) acc += (int)p[t] * kk[t];
            px[j] = clip8(acc);
        }
        store_px(dst + ((size_t)c * it.h + y) * W + x0, px, valid, all);
    }
}

__global__ __launch_bounds__(RS_THREADS) void resize_cols_kernel(const cosy_resize_item_t* __restrict__ items, int C, int H, int W, int max_h,
                                                                 const int* __restrict__ tables, long n_tables, unsigned char* __restrict__ out,
                                                                 const unsigned char* __restrict__ ws) {
    const int i = blockIdx.z;
    const ResizeItem it = resize_load(items, i, H, W, max_h, tables, n_tables);
    if (!it.ok || (it.vks == 0 && it.hks != 0)) return;       // rows only: resize_rows_kernel wrote `out`
    const int yy = blockIdx.y * RS_ROWS + __builtin_amdgcn_readfirstlane(threadIdx.x / RS_LANES);
    const int x0 = (blockIdx.x * RS_LANES + (threadIdx.x % RS_LANES)) * RS_PX;
    if (yy >= H || x0 >= W) return;
    const unsigned char* in = it.hks ? ws + (size_t)i * C * max_h * W : it.src;          // C planes of h x W either way
    int ymin = yy, ymax = 1;                                  // no vertical pass either: a copy, one tap of weight 2^22
    const int* kk = nullptr;
    if (it.vks) {
        ymin = it.vb[2 * yy]; ymax = it.vb[2 * yy + 1];
        if (!bounds_ok(ymin, ymax, it.vks, it.h)) return;
        kk = it.vk + (size_t)yy * it.vks;
    }
    bool valid[RS_PX];
#pragma unroll
    for (int j = 0; j < RS_PX; ++j) valid[j] = x0 + j < W;
    const bool all = valid[RS_PX - 1];
    for (int c = 0; c < C; ++c) {
        const unsigned char* col = in + ((size_t)c * it.h + ymin) * W + x0;
        int acc[RS_PX];
#pragma unroll
        for (int j = 0; j < RS_PX; ++j) acc[j] = 1 << (RS_BITS - 1);
        for (int t = 0; t < ymax; ++t) {
            const int kv = kk ? kk[t] : 1 << RS_BITS;
            const unsigned char* p = col + (size_t)t * W;
            if (all && ((uintptr_t)p & 3) == 0) {
                const unsigned v = *reinterpret_cast<const unsigned*>(p);
#pragma unroll
                for (int j = 0; j < RS_PX; ++j) acc[j] += (int)((v >> (8 * j)) & 255u) * kv;
            } else {
#pragma unroll
                for (int j = 0; j < RS_PX; ++j)
                    if (valid[j]) acc[j] += (int)p[j] * kv;
            }
        }
        unsigned px[RS_PX];
#pragma unroll
        for (int j = 0; j < RS_PX; ++j) px[j] = clip8(acc[j]);
        store_px(out + (((size_t)i * C + c) * H + yy) * W + x0, px, valid, all);
    }
}

}  // namespace
}  // namespace cosy

using namespace cosy;

extern "C" {

int cosy_resize_ksize(int in, int out, int filter) {
    double s;
    COSY_REQUIRE(filter_support(filter, s), "cosy_resize_ksize: filter=%d is neither COSY_RESIZE_BILINEAR nor COSY_RESIZE_BICUBIC", filter);
    COSY_REQUIRE(in >= 1 && out >= 1 && in <= RS_MAX_AXIS && out <= RS_MAX_AXIS, "cosy_resize_ksize: in=%d out=%d (1 .. %d)", in, out, RS_MAX_AXIS);
    double filterscale = (double)in / out;
    if (filterscale < 1.0) filterscale = 1.0;
    const double support = s * filterscale;
    return (int)ceil(support) * 2 + 1;
}

// Pillow's precompute_coeffs + normalize_coeffs_8bpc (src/libImaging/Resample.c), restated: the weights are summed in index order, one
// addition at a time, and divided one by one.
int cosy_resize_coeffs(int in, int out, int filter, int* bounds, int* k, size_t capacity) {
    const int ksize = cosy_resize_ksize(in, out, filter);
    if (ksize < 0) return ksize;
    COSY_REQUIRE_PTR("cosy_resize_coeffs", bounds); COSY_REQUIRE_PTR("cosy_resize_coeffs", k);
    if (capacity < (size_t)out * ksize) {
        set_error("cosy_resize_coeffs: capacity=%zu < out * ksize = %zu", capacity, (size_t)out * ksize);
        return COSY_ESIZE;
    }
    double s = 0.0;
    filter_support(filter, s);
    double (*f)(double) = filter == COSY_RESIZE_BILINEAR ? bilinear_filter : bicubic_filter;
    const double scale = (double)in / out;
    double filterscale = scale;
    if (filterscale < 1.0) filterscale = 1.0;
    const double support = s * filterscale;
    const double ss = 1.0 / filterscale;
    std::vector<double> w(ksize);
    for (int xx = 0; xx < out; ++xx) {
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in) xmax = in;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            w[x] = f((x + xmin - center + 0.5) * ss);
            ww += w[x];
        }
        int* kx = k + (size_t)xx * ksize;
        for (int x = 0; x < ksize; ++x) {
            double v = 0.0;
            if (x < xmax) v = ww != 0.0 ? w[x] / ww : w[x];
            kx[x] = v < 0 ? (int)(-0.5 + v * (1 << RS_BITS)) : (int)(0.5 + v * (1 << RS_BITS));
        }
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
    return ksize;
}

size_t cosy_resize_workspace_bytes(int n, int C, int max_h, int W) {
    if (n <= 0 || C <= 0 || max_h <= 0 || W <= 0) return 0;
    return ((size_t)n * C * max_h * W + 255) / 256 * 256;
}

int cosy_resize_u8(const cosy_resize_item_t* items, int n, int C, int H, int W, int max_h, const int* tables, long n_tables, unsigned char* out,
                   void* workspace, size_t workspace_bytes, cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    COSY_REQUIRE(n >= 0 && C >= 1 && H >= 1 && W >= 1 && max_h >= 1 && n_tables >= 0, "cosy_resize_u8: n=%d C=%d H=%d W=%d max_h=%d n_tables=%ld", n,
                 C, H, W, max_h, n_tables);
    COSY_REQUIRE(n <= COSY_MAX_GRID_Y, "cosy_resize_u8: n=%d exceeds %d images per call", n, COSY_MAX_GRID_Y);
    COSY_REQUIRE(cdiv(max_h, RS_ROWS) <= COSY_MAX_GRID_Y && cdiv(H, RS_ROWS) <= COSY_MAX_GRID_Y && (long)C * max_h * W < (1L << 31) &&
                     (long)C * H * W < (1L << 31),
                 "cosy_resize_u8: images of %d x %d x %d (rows up to %d) are too large", C, H, W, max_h);
    if (n == 0) return COSY_OK;
    COSY_REQUIRE_PTR("cosy_resize_u8", items); COSY_REQUIRE_PTR("cosy_resize_u8", tables);
    COSY_REQUIRE_PTR("cosy_resize_u8", out); COSY_REQUIRE_PTR("cosy_resize_u8", workspace);
    COSY_REQUIRE(workspace_bytes >= cosy_resize_workspace_bytes(n, C, max_h, W), "cosy_resize_u8: workspace_bytes=%zu < %zu", workspace_bytes,
                 cosy_resize_workspace_bytes(n, C, max_h, W));
    COSY_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)items & 7) == 0 && ((uintptr_t)tables & 3) == 0,
                 "cosy_resize_u8: workspace not 16-byte, items not 8-byte or tables not 4-byte aligned");
    hipLaunchKernelGGL(resize_rows_kernel, dim3(cdiv(W, RS_TILE_W), cdiv(max_h, RS_ROWS), n), dim3(RS_THREADS), 0, s, items, C, H, W, max_h, tables,
                       n_tables, out, (unsigned char*)workspace);
    COSY_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(resize_cols_kernel, dim3(cdiv(W, RS_TILE_W), cdiv(H, RS_ROWS), n), dim3(RS_THREADS), 0, s, items, C, H, W, max_h, tables,
                       n_tables, out, (const unsigned char*)workspace);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

}  // extern "C"
