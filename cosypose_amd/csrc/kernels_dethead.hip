// The detector's heads on the matrix pipe: every layer of Mask R-CNN's RPN head, box head + predictor and mask head +
// predictor is ONE implicit GEMM,  out[cout][pixel] = sum over (tap, channel) of w[cout][tap][channel] * x[pixel + tap][channel]:
//   * 3x3 conv (pad 1, stride 1): 9 taps; 1x1 conv: 1 tap; a linear layer: the 1x1 case on maps of one cell;
//   * ConvTranspose2d(k=2, s=2): a 1x1 GEMM to 4 C_out columns (o, dy, dx) whose epilogue scatters column (o, dy, dx) of cell (y, x) to (o, 2y+dy, 2x+dx).
// Activations are ROWS: row = (level, image, y, x) in that order, C_in contiguous channels of the storage type T (NHWC; a linear layer's row is
// its input vector).  cosy_head_pack makes rows out of a contiguous NCHW float32 map.  Weights arrive packed in fragment order (cosyhip.h).
//
// The GEMM body, its summation order and its epilogue are stated once, in dethead_device.h, which kernels_dettrunk.hip instantiates too;
// this file holds the heads' instantiation (stride 1, bias + ReLU), the packers and the entry points.
#include "dethead_device.h"

namespace cosy {
namespace {

using namespace headgemm;

// the launcher's row threshold and its large tile, under the names the heads' entry points report them by (cosy_head_big_rows,
// cosy_head_max_tile_rows); dethead_device.h holds the one definition both instantiations compile
constexpr int HEAD_BIG_ROWS = 1024;
constexpr int HEAD_MT_BIG = 4, HEAD_NT_BIG = 4;
static_assert(HEAD_BIG_ROWS == TILE_BIG_ROWS && HEAD_MT_BIG == TILE_MT_BIG && HEAD_NT_BIG == TILE_NT_BIG, "the heads report the shared launcher's tiles");

// (B,C,HW) float32 -> rows (B HW, C) of T through a 32-channel x 64-pixel LDS tile: reads run along the pixels, writes along the channels
template <typename T> __global__ __launch_bounds__(HEAD_THREADS) void head_pack_kernel(const float* __restrict__ in, T* __restrict__ out, int C, int HW) {
    __shared__ float tile[32][65];
    const int t = threadIdx.x, p0 = blockIdx.x * 64, c0 = blockIdx.y * 32;
    const long b = blockIdx.z;
    {
        const int p = t & 63, cc = t >> 6;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int c = c0 + cc + 4 * i;
            if (c < C && p0 + p < HW) tile[cc + 4 * i][p] = in[(b * C + c) * HW + p0 + p];
        }
    }
    __syncthreads();
    const int p = t >> 2, c8 = (t & 3) * 8;
    if (p0 + p < HW && c0 + c8 < C) {                          // C is a multiple of 8
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = tile[c8 + k][p];
        T* dst = out + (b * HW + p0 + p) * C + c0 + c8;
        put4(dst, v); put4(dst + 4, v + 4);
    }
}

// HW = 1: the map is its own rows; only the type changes
template <typename T> __global__ __launch_bounds__(HEAD_THREADS) void head_cast_kernel(const float* __restrict__ in, T* __restrict__ out, long n4) {
    const long i = (long)blockIdx.x * HEAD_THREADS + threadIdx.x;
    if (i >= n4) return;
    const f32x4 u = ((const f32x4*)in)[i];
    const float v[4] = {u[0], u[1], u[2], u[3]};
    put4(out + 4 * i, v);
}

template <typename T> int launch_head_conv(const cosy_head_layer_t& a, int M, hipStream_t s) {
    const conv_grid_t c = conv_grid<T>(a, M);
    COSY_REQUIRE(c.blocks <= 0x7fffffffL, "cosy_head_conv: %d rows x c_out=%d need more than 2^31 - 1 workgroups", M, a.c_out);
    const dim3 grid((unsigned)c.blocks);
    const bool big_m = c.big_m, big_n = c.big_n;
    const int KBn = c.KBn, n_tiles = c.n_tiles, ng = c.n_groups;
    if (big_m && big_n) hipLaunchKernelGGL((conv_gemm_kernel<T, HEAD_MT_BIG, HEAD_NT_BIG, HeadPolicy>), grid, dim3(HEAD_THREADS), 0, s, a, M, KBn, n_tiles, ng, no_epi_t{});
    else if (big_m) hipLaunchKernelGGL((conv_gemm_kernel<T, HEAD_MT_BIG, 1, HeadPolicy>), grid, dim3(HEAD_THREADS), 0, s, a, M, KBn, n_tiles, ng, no_epi_t{});
    else if (big_n) hipLaunchKernelGGL((conv_gemm_kernel<T, 1, HEAD_NT_BIG, HeadPolicy>), grid, dim3(HEAD_THREADS), 0, s, a, M, KBn, n_tiles, ng, no_epi_t{});
    else hipLaunchKernelGGL((conv_gemm_kernel<T, 1, 1, HeadPolicy>), grid, dim3(HEAD_THREADS), 0, s, a, M, KBn, n_tiles, ng, no_epi_t{});
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

}  // namespace
}  // namespace cosy

using namespace cosy;

extern "C" {

int cosy_head_big_rows(void) { return HEAD_BIG_ROWS; }
int cosy_head_max_tile_rows(void) { return 64 * HEAD_MT_BIG; }

int cosy_head_pack(const float* in, void* rows, int B, int C, int HW, int dtype, cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    COSY_REQUIRE(dtype == COSY_F32 || dtype == COSY_BF16 || dtype == COSY_F16, "cosy_head_pack: dtype=%d is not COSY_F32, COSY_BF16 or COSY_F16", dtype);
    COSY_REQUIRE(B >= 0 && HW >= 1, "cosy_head_pack: B=%d must be >= 0 and HW=%d >= 1", B, HW);
    COSY_REQUIRE(C >= 8 && C % 8 == 0, "cosy_head_pack: C=%d must be a positive multiple of 8", C);
    COSY_REQUIRE((long)B * HW <= HEAD_MAX_ROWS, "cosy_head_pack: B HW = %ld rows exceed 2^30", (long)B * HW);
    if (B == 0) return COSY_OK;
    COSY_REQUIRE_PTR("cosy_head_pack", in); COSY_REQUIRE_PTR("cosy_head_pack", rows);
    COSY_REQUIRE(((uintptr_t)in & 15) == 0 && ((uintptr_t)rows & 15) == 0, "cosy_head_pack: in and rows must be 16-byte aligned");
    if (HW == 1) {
        const long n4 = (long)B * C / 4;
        COSY_REQUIRE((long)B * C <= (1L << 38), "cosy_head_pack: B C = %ld elements exceed 2^38", (long)B * C);
        COSY_DISPATCH_STMT(dtype, hipLaunchKernelGGL(head_cast_kernel<T>, dim3(cdiv(n4, HEAD_THREADS)), dim3(HEAD_THREADS), 0, s, in, (T*)rows, n4));
    } else {
        COSY_REQUIRE(B <= COSY_MAX_GRID_Y && cdiv(C, 32) <= COSY_MAX_GRID_Y, "cosy_head_pack: B=%d maps and C=%d / 32 channel groups must not exceed %d",
                     B, C, COSY_MAX_GRID_Y);
        COSY_DISPATCH_STMT(dtype, hipLaunchKernelGGL(head_pack_kernel<T>, dim3(cdiv(HW, 64), cdiv(C, 32), B), dim3(HEAD_THREADS), 0, s, in, (T*)rows, C, HW));
    }
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

int cosy_head_conv(const cosy_head_layer_t* layer, cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    COSY_REQUIRE_PTR("cosy_head_conv", layer);
    const cosy_head_layer_t& a = *layer;
    COSY_REQUIRE(a.dtype == COSY_F32 || a.dtype == COSY_BF16 || a.dtype == COSY_F16, "cosy_head_conv: dtype=%d is not COSY_F32, COSY_BF16 or COSY_F16", a.dtype);
    COSY_REQUIRE(a.ksize == 1 || a.ksize == 3, "cosy_head_conv: ksize=%d must be 1 or 3", a.ksize);
    COSY_REQUIRE(a.c_in >= 8 && a.c_in % 8 == 0, "cosy_head_conv: the reduction length c_in=%d must be a positive multiple of 8", a.c_in);
    COSY_REQUIRE(a.c_out >= 1, "cosy_head_conv: c_out=%d must be >= 1", a.c_out);
    COSY_REQUIRE(a.store >= COSY_HEAD_STORE_ROWS && a.store <= COSY_HEAD_STORE_DECONV_NCHW, "cosy_head_conv: store=%d is not a COSY_HEAD_STORE_* value", a.store);
    COSY_REQUIRE(a.relu == 0 || a.relu == 1, "cosy_head_conv: relu=%d must be 0 or 1", a.relu);
    if (a.store == COSY_HEAD_STORE_ROWS)
        COSY_REQUIRE(a.c_out % 8 == 0, "cosy_head_conv: c_out=%d stored as rows must be a multiple of 8 (the next layer's reduction length)", a.c_out);
    if (a.store == COSY_HEAD_STORE_DECONV_ROWS || a.store == COSY_HEAD_STORE_DECONV_NCHW) {
        COSY_REQUIRE(a.ksize == 1 && a.c_out % 4 == 0, "cosy_head_conv: a deconvolution is a 1x1 layer of 4 C_out columns, got ksize=%d, c_out=%d", a.ksize, a.c_out);
        COSY_REQUIRE(a.store == COSY_HEAD_STORE_DECONV_NCHW || a.c_out % 32 == 0, "cosy_head_conv: c_out / 4 = %d stored as rows must be a multiple of 8", a.c_out / 4);
    }
    if (a.store == COSY_HEAD_STORE_NCHW) COSY_REQUIRE(a.n_split >= 0 && a.n_split <= a.c_out, "cosy_head_conv: n_split=%d must lie in [0, c_out=%d]", a.n_split, a.c_out);
    COSY_REQUIRE(a.n_levels >= 1 && a.n_levels <= COSY_RPN_MAX_LEVELS, "cosy_head_conv: n_levels=%d must lie in [1, %d]", a.n_levels, COSY_RPN_MAX_LEVELS);
    COSY_REQUIRE(a.row_start[0] == 0, "cosy_head_conv: row_start[0]=%d must be 0", a.row_start[0]);
    for (int l = 0; l < a.n_levels; ++l) {
        COSY_REQUIRE(a.H[l] >= 1 && a.W[l] >= 1 && (long)a.H[l] * a.W[l] <= HEAD_MAX_ROWS, "cosy_head_conv: level %d is %d x %d cells", l, a.H[l], a.W[l]);
        const long n = (long)a.row_start[l + 1] - a.row_start[l];
        COSY_REQUIRE(n >= 0 && n % ((long)a.H[l] * a.W[l]) == 0, "cosy_head_conv: level %d owns %ld rows, not whole maps of %d x %d cells", l, n, a.H[l], a.W[l]);
    }
    const int M = a.row_start[a.n_levels];
    COSY_REQUIRE(M <= HEAD_MAX_ROWS, "cosy_head_conv: %d rows exceed 2^30", M);
    if (M == 0) return COSY_OK;
    COSY_REQUIRE_PTR("cosy_head_conv", a.x); COSY_REQUIRE_PTR("cosy_head_conv", a.w); COSY_REQUIRE_PTR("cosy_head_conv", a.bias); COSY_REQUIRE_PTR("cosy_head_conv", a.out);
    COSY_REQUIRE(a.store != COSY_HEAD_STORE_NCHW || a.n_split == a.c_out || a.out1 != nullptr, "cosy_head_conv: null out1 with n_split=%d < c_out=%d", a.n_split, a.c_out);
    COSY_REQUIRE(((uintptr_t)a.x & 15) == 0 && ((uintptr_t)a.w & 15) == 0 && ((uintptr_t)a.out & 15) == 0, "cosy_head_conv: x, w and out must be 16-byte aligned");
    return COSY_DISPATCH_T(a.dtype, launch_head_conv<T>(a, M, s));
}

}  // extern "C"
