// The detector's trunk on the matrix pipe: every convolution of the ResNet-50 body and of the FPN is the heads' implicit
// GEMM (dethead_device.h) with a stride of 1 or 2 on the taps and the trunk's epilogue: FrozenBatchNorm as one fmaf(acc, scale, shift), the
// bottleneck's shortcut or the FPN's nearest-upsampled coarser level as one rounded add, ReLU, the conversion to the store's type.
//   * cosy_trunk_conv: out rows = the OUTPUT cells, Ho = (H - 1) / stride + 1; output cell (y, x) reads the input cells (stride y + dy, stride x + dx),
//     a tap outside the map feeds +0.0 and its address is never formed.
//   * cosy_trunk_stem_pack: the 7x7 stride-2 pad-3 stem's taps as rows of 152 = 7 x 7 x 3 + 5 elements, so that the stem is a one-tap GEMM.
//   * cosy_trunk_maxpool: 3x3 stride 2 pad 1 over rows, padding -inf, torch's NaN rule.
// Activations are rows (image, y, x) of contiguous channels in the storage type, as in the heads.
#include "dethead_device.h"

namespace cosy {
namespace {

using namespace headgemm;

constexpr int STEM_K = 7, STEM_C = 3, STEM_ROW = 152;          // 147 taps x channels, padded to a multiple of 8

template <typename T, int STRIDE> int launch_trunk_conv(const cosy_head_layer_t& a, const conv_epi_t& e, int M, hipStream_t s) {
    const conv_grid_t c = conv_grid<T>(a, M);
    COSY_REQUIRE(c.blocks <= 0x7fffffffL, "cosy_trunk_conv: %d rows x c_out=%d need more than 2^31 - 1 workgroups", M, a.c_out);
    const dim3 grid((unsigned)c.blocks);
    if (c.big_m && c.big_n) hipLaunchKernelGGL((conv_gemm_kernel<T, TILE_MT_BIG, TILE_NT_BIG, ConvPolicy<STRIDE, true>>), grid, dim3(HEAD_THREADS), 0, s, a, M, c.KBn, c.n_tiles, c.n_groups, e);
    else if (c.big_m) hipLaunchKernelGGL((conv_gemm_kernel<T, TILE_MT_BIG, 1, ConvPolicy<STRIDE, true>>), grid, dim3(HEAD_THREADS), 0, s, a, M, c.KBn, c.n_tiles, c.n_groups, e);
    else if (c.big_n) hipLaunchKernelGGL((conv_gemm_kernel<T, 1, TILE_NT_BIG, ConvPolicy<STRIDE, true>>), grid, dim3(HEAD_THREADS), 0, s, a, M, c.KBn, c.n_tiles, c.n_groups, e);
    else hipLaunchKernelGGL((conv_gemm_kernel<T, 1, 1, ConvPolicy<STRIDE, true>>), grid, dim3(HEAD_THREADS), 0, s, a, M, c.KBn, c.n_tiles, c.n_groups, e);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

// one thread: 8 consecutive elements of one output row (19 groups per row); element (ky 7 + kx) 3 + c = images[b, c, 2y - 3 + ky, 2x - 3 + kx]
template <typename T> __global__ __launch_bounds__(HEAD_THREADS) void stem_pack_kernel(const float* __restrict__ in, T* __restrict__ out, int H, int W, int Ho, int Wo, long n) {
    const long i = (long)blockIdx.x * HEAD_THREADS + threadIdx.x;
    if (i >= n) return;
    const long row = i / (STEM_ROW / 8);
    const int e0 = (int)(i - row * (STEM_ROW / 8)) * 8;
    const int x = (int)(row % Wo), y = (int)((row / Wo) % Ho);
    const long b = row / ((long)Wo * Ho);
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int e = e0 + k, tap = e / STEM_C, c = e - tap * STEM_C, ky = tap / STEM_K, kx = tap - ky * STEM_K;
        const int iy = 2 * y - 3 + ky, ix = 2 * x - 3 + kx;
        v[k] = 0.f;
        if (e < STEM_K * STEM_K * STEM_C && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) v[k] = in[((b * STEM_C + c) * H + iy) * W + ix];
    }
    T* dst = out + row * STEM_ROW + e0;
    put4(dst, v); put4(dst + 4, v + 4);
}

// one thread: 8 consecutive channels of one output cell; the taps (ky, kx) ascending, torch's rule: v > m || isnan(v) takes v
template <typename T> __global__ __launch_bounds__(HEAD_THREADS) void maxpool_kernel(const T* __restrict__ in, T* __restrict__ out, int H, int W, int Ho, int Wo, int C, long n) {
    const long i = (long)blockIdx.x * HEAD_THREADS + threadIdx.x;
    if (i >= n) return;
    const int C8 = C / 8;
    const long row = i / C8;
    const int c0 = (int)(i - row * C8) * 8;
    const int x = (int)(row % Wo), y = (int)((row / Wo) % Ho);
    const long b = row / ((long)Wo * Ho);
    float m[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) m[k] = -__builtin_inff();
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = 2 * y - 1 + ky;
        if ((unsigned)iy >= (unsigned)H) continue;
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = 2 * x - 1 + kx;
            if ((unsigned)ix >= (unsigned)W) continue;
            float v[8];
            load8(in + ((b * H + iy) * W + ix) * C + c0, v);
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (v[k] > m[k] || v[k] != v[k]) m[k] = v[k];
        }
    }
    T* dst = out + row * C + c0;                               // values of the type go back unchanged: the conversion is exact
    put4(dst, m); put4(dst + 4, m + 4);
}

}  // namespace
}  // namespace cosy

using namespace cosy;

extern "C" {

int cosy_trunk_conv(const cosy_head_layer_t* layer, int stride, const float* scale, const void* residual, int res_H, int res_W, cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    COSY_REQUIRE_PTR("cosy_trunk_conv", layer);
    const cosy_head_layer_t& a = *layer;
    COSY_REQUIRE(a.dtype == COSY_F32 || a.dtype == COSY_BF16 || a.dtype == COSY_F16, "cosy_trunk_conv: dtype=%d is not COSY_F32, COSY_BF16 or COSY_F16", a.dtype);
    COSY_REQUIRE(a.ksize == 1 || a.ksize == 3, "cosy_trunk_conv: ksize=%d must be 1 or 3", a.ksize);
    COSY_REQUIRE(stride == 1 || stride == 2, "cosy_trunk_conv: stride=%d must be 1 or 2", stride);
    COSY_REQUIRE(a.c_in >= 8 && a.c_in % 8 == 0, "cosy_trunk_conv: the reduction length c_in=%d must be a positive multiple of 8", a.c_in);
    COSY_REQUIRE(a.c_out >= 1, "cosy_trunk_conv: c_out=%d must be >= 1", a.c_out);
    COSY_REQUIRE(a.store == COSY_HEAD_STORE_ROWS || a.store == COSY_HEAD_STORE_NCHW, "cosy_trunk_conv: store=%d is not COSY_HEAD_STORE_ROWS or COSY_HEAD_STORE_NCHW", a.store);
    COSY_REQUIRE(a.relu == 0 || a.relu == 1, "cosy_trunk_conv: relu=%d must be 0 or 1", a.relu);
    if (a.store == COSY_HEAD_STORE_ROWS)
        COSY_REQUIRE(a.c_out % 8 == 0, "cosy_trunk_conv: c_out=%d stored as rows must be a multiple of 8 (the next layer's reduction length)", a.c_out);
    else
        COSY_REQUIRE(a.n_split == a.c_out, "cosy_trunk_conv: n_split=%d must equal c_out=%d (the trunk has no sibling layers)", a.n_split, a.c_out);
    COSY_REQUIRE(a.n_levels >= 1 && a.n_levels <= COSY_RPN_MAX_LEVELS, "cosy_trunk_conv: n_levels=%d must lie in [1, %d]", a.n_levels, COSY_RPN_MAX_LEVELS);
    COSY_REQUIRE(stride == 1 || a.n_levels == 1, "cosy_trunk_conv: stride=2 takes one level, got n_levels=%d", a.n_levels);
    COSY_REQUIRE(residual == nullptr || a.n_levels == 1, "cosy_trunk_conv: a residual takes one level, got n_levels=%d", a.n_levels);
    COSY_REQUIRE(a.row_start[0] == 0, "cosy_trunk_conv: row_start[0]=%d must be 0", a.row_start[0]);
    for (int l = 0; l < a.n_levels; ++l) {
        COSY_REQUIRE(a.H[l] >= 1 && a.W[l] >= 1 && (long)a.H[l] * a.W[l] <= HEAD_MAX_ROWS, "cosy_trunk_conv: level %d is %d x %d cells", l, a.H[l], a.W[l]);
        const long n = (long)a.row_start[l + 1] - a.row_start[l];
        COSY_REQUIRE(n >= 0 && n % ((long)a.H[l] * a.W[l]) == 0, "cosy_trunk_conv: level %d owns %ld rows, not whole maps of %d x %d cells", l, n, a.H[l], a.W[l]);
    }
    const int M_in = a.row_start[a.n_levels];
    COSY_REQUIRE(M_in <= HEAD_MAX_ROWS, "cosy_trunk_conv: %d rows exceed 2^30", M_in);
    // the rows the launch owns: the output cells
    const int Ho = (a.H[0] - 1) / stride + 1, Wo = (a.W[0] - 1) / stride + 1;
    const int M = stride == 1 ? M_in : (int)((long)M_in / ((long)a.H[0] * a.W[0]) * Ho * Wo);
    if (residual != nullptr) {
        COSY_REQUIRE(res_H >= 1 && res_W >= 1 && (long)res_H * res_W <= HEAD_MAX_ROWS, "cosy_trunk_conv: the residual's maps are %d x %d cells", res_H, res_W);
        COSY_REQUIRE(a.c_out % 8 == 0, "cosy_trunk_conv: c_out=%d with a residual must be a multiple of 8 (the residual's rows)", a.c_out);
        COSY_REQUIRE((long)M_in / ((long)a.H[0] * a.W[0]) * res_H * res_W <= HEAD_MAX_ROWS, "cosy_trunk_conv: the residual's rows exceed 2^30");
    }
    if (M == 0) return COSY_OK;
    COSY_REQUIRE_PTR("cosy_trunk_conv", a.x); COSY_REQUIRE_PTR("cosy_trunk_conv", a.w); COSY_REQUIRE_PTR("cosy_trunk_conv", a.bias); COSY_REQUIRE_PTR("cosy_trunk_conv", a.out);
    COSY_REQUIRE(((uintptr_t)a.x & 15) == 0 && ((uintptr_t)a.w & 15) == 0 && ((uintptr_t)a.out & 15) == 0, "cosy_trunk_conv: x, w and out must be 16-byte aligned");
    COSY_REQUIRE(((uintptr_t)residual & 15) == 0 && ((uintptr_t)scale & 3) == 0, "cosy_trunk_conv: residual must be 16-byte and scale 4-byte aligned");
    conv_epi_t e;
    e.scale = scale; e.residual = residual; e.res_H = residual ? res_H : 1; e.res_W = residual ? res_W : 1;
    e.sy = (float)e.res_H / (float)Ho; e.sx = (float)e.res_W / (float)Wo;
    if (stride == 1) return COSY_DISPATCH_T(a.dtype, (launch_trunk_conv<T, 1>(a, e, M, s)));
    return COSY_DISPATCH_T(a.dtype, (launch_trunk_conv<T, 2>(a, e, M, s)));
}

int cosy_trunk_stem_pack(const float* images, void* rows, int B, int H, int W, int dtype, cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    COSY_REQUIRE(dtype == COSY_F32 || dtype == COSY_BF16 || dtype == COSY_F16, "cosy_trunk_stem_pack: dtype=%d is not COSY_F32, COSY_BF16 or COSY_F16", dtype);
    COSY_REQUIRE(B >= 0 && H >= 1 && W >= 1, "cosy_trunk_stem_pack: B=%d must be >= 0 and the images %d x %d at least one pixel", B, H, W);
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    COSY_REQUIRE((long)B * Ho * Wo <= HEAD_MAX_ROWS, "cosy_trunk_stem_pack: B Ho Wo = %ld rows exceed 2^30", (long)B * Ho * Wo);
    if (B == 0) return COSY_OK;
    COSY_REQUIRE_PTR("cosy_trunk_stem_pack", images); COSY_REQUIRE_PTR("cosy_trunk_stem_pack", rows);
    COSY_REQUIRE(((uintptr_t)images & 3) == 0 && ((uintptr_t)rows & 15) == 0, "cosy_trunk_stem_pack: images must be 4-byte and rows 16-byte aligned");
    const long n = (long)B * Ho * Wo * (STEM_ROW / 8);
    COSY_REQUIRE((n + HEAD_THREADS - 1) / HEAD_THREADS <= 0x7fffffffL, "cosy_trunk_stem_pack: too many workgroups");
    COSY_DISPATCH_STMT(dtype, hipLaunchKernelGGL(stem_pack_kernel<T>, dim3((unsigned)((n + HEAD_THREADS - 1) / HEAD_THREADS)), dim3(HEAD_THREADS), 0, s, images, (T*)rows, H, W, Ho, Wo, n));
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

int cosy_trunk_maxpool(const void* x, void* out, int B, int H, int W, int C, int dtype, cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    COSY_REQUIRE(dtype == COSY_F32 || dtype == COSY_BF16 || dtype == COSY_F16, "cosy_trunk_maxpool: dtype=%d is not COSY_F32, COSY_BF16 or COSY_F16", dtype);
    COSY_REQUIRE(B >= 0 && H >= 1 && W >= 1, "cosy_trunk_maxpool: B=%d must be >= 0 and the maps %d x %d at least one cell", B, H, W);
    COSY_REQUIRE(C >= 8 && C % 8 == 0, "cosy_trunk_maxpool: C=%d must be a positive multiple of 8", C);
    COSY_REQUIRE((long)B * H * W <= HEAD_MAX_ROWS, "cosy_trunk_maxpool: B H W = %ld rows exceed 2^30", (long)B * H * W);
    if (B == 0) return COSY_OK;
    COSY_REQUIRE_PTR("cosy_trunk_maxpool", x); COSY_REQUIRE_PTR("cosy_trunk_maxpool", out);
    COSY_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)out & 15) == 0, "cosy_trunk_maxpool: x and out must be 16-byte aligned");
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const long n = (long)B * Ho * Wo * (C / 8);
    COSY_REQUIRE((n + HEAD_THREADS - 1) / HEAD_THREADS <= 0x7fffffffL, "cosy_trunk_maxpool: too many workgroups");
    COSY_DISPATCH_STMT(dtype, hipLaunchKernelGGL(maxpool_kernel<T>, dim3((unsigned)((n + HEAD_THREADS - 1) / HEAD_THREADS)), dim3(HEAD_THREADS), 0, s, (const T*)x, (T*)out, H, W, Ho, Wo, C, n));
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

}  // extern "C"
