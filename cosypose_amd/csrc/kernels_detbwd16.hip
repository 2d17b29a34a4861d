// The backward of the detector's trunk and heads (section 32) on bfloat16 rows: ONE set of kernels, as kernels_detbwd.hip
// is for float32.  The parameters stay float32 (the master weights); the rows the forward keeps, the gradient rows and both packed weights are
// bfloat16, every accumulation is float32.
//   * weight_pack16_kernel: float32 parameters in torchvision's layout (one layer, or two siblings of one GEMM, or ConvTranspose2d(2, 2)) -> fwd,
//     the bytes of the host packing of bf16(w) that cosy_head_conv / cosy_trunk_conv read at COSY_BF16, fwd_bias, and bwd, the transposed,
//     tap-flipped packing of ws = bf16(fl32(w scale[o])) (the heads: no scale) in the same 16-bit fragment order.
//   * grad_pack16_kernel: the losses' NCHW float32 gradients (one tensor, or a sibling pair) -> bfloat16 rows, the pad columns +0.0.
//   * the data gradient is detbwd_device.h's kernel on bfloat16 rows: one v_mfma_f32_16x16x32_bf16 per (block of 32 o, live tap); the heads' first
//     layers store its accumulator as float32 NCHW; the deconvolution's is dethead_device.h's conv_gemm_kernel under DeconvGradPolicyOf<bf16_t>.
//   * wgrad16_kernel: dW[o][tap][c] = sum over OUTPUT cells of g[cell][o] x[cell + tap][c] with the CELLS as the k dimension of
//     v_mfma_f32_16x16x32_bf16.  The instruction wants eight consecutive cells of ONE channel per lane for both operands; the rows are stored
//     cell-major.  A wave loads whole row segments (16 bytes: eight channels of one cell per lane), lays 32 cells x 16 channels images in LDS and
//     reads them back transposed with ds_read_b64_tr_b16.  The image: a cell's 16 channels are 32 contiguous bytes, eight cells a 256-byte group,
//     and every group is followed by 128 bytes of pad (group stride 384).  One transposed read of a 32-lane half takes cells 8 G .. 8 G + 3 of
//     two neighbouring groups G: 2 x 128 contiguous bytes that start 384 bytes apart, i.e. banks [0, 32) and [32, 64) (or the reverse): all 64
//     banks once, no conflict by the bank rule.  Every wave owns its images: no barrier, only wave-level ordering of its own LDS traffic, and
//     EXEC is all ones at every transposed read (a wave past the last tile leaves as a whole; cells past the slab, taps outside the map and
//     channels past the row are staged as +0.0, never masked).
//     Slabs, partial tiles, the ascending second pass and the one scale[o] product are kernels_detbwd.hip's (same workspace rule).
// No atomics: equal inputs give equal bits.
#include "detbwd_device.h"

namespace cosy {
namespace {

using namespace headgemm;
using namespace detbwd;

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

constexpr int WG_CELLS = 32;                 // cells of one k-step
constexpr int WG_GROUP = 384;                // bytes from one 8-cell group of an image to the next: 8 x 32 bytes of data, 128 of pad
constexpr int WG_IMAGE = (WG_CELLS / 8) * WG_GROUP;      // one image: 32 cells x 16 channels

__device__ __forceinline__ int image_off(int cell) { return WG_GROUP * (cell >> 3) + 32 * (cell & 7); }

// the wave's own LDS writes become visible to its own (cross-lane) reads, and the other way round: orders, emits no barrier instruction
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the MFMA operand of one image: lane (G = lane >> 4, i = lane & 15) gets channel i of the cells 8 G .. 8 G + 7.  rd: the lane's address of the
// first read, 384 G + 32 q + 8 p with i = 4 q + p (row q of the block, columns 4 p .. 4 p + 3); the second read is four cells (128 bytes) on
__device__ __forceinline__ bf16x8 image_frag(const unsigned char* image, int rd) {
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(image + rd));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(image + rd + 128));
    return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// cosy_head_weight_pack16 / cosy_trunk_weight_pack16: the same launch with bfloat16 packings (32 of the reduction per block, eight elements per lane);
// scale: one float32 product, then ONE rounding to bfloat16 (detbwd_device.h's weight_pack_element)
__global__ __launch_bounds__(HEAD_THREADS) void weight_pack16_kernel(const float* __restrict__ w0, const float* __restrict__ b0, const float* __restrict__ w1,
                                                                     const float* __restrict__ b1, const float* __restrict__ scale, int ksize, int C, int n0, int n1,
                                                                     bf16_t* __restrict__ fwd, float* __restrict__ fwd_bias, bf16_t* __restrict__ bwd, long n_fwd,
                                                                     long n_bwd, int n_bias) {
    weight_pack_element<bf16_t>((long)blockIdx.x * HEAD_THREADS + threadIdx.x, w0, b0, w1, b1, scale, ksize, C, n0, n1, fwd, fwd_bias, bwd, n_fwd, n_bwd, n_bias);
}

// NCHW float32 (B, n0, HW) and (B, n1, HW) -> bfloat16 rows (B HW, GP): the columns of the first, then of the second, then +0.0; a null tensor is
// zeros.  One thread: eight columns of one cell; neighbouring threads take neighbouring cells of the same columns
__global__ __launch_bounds__(HEAD_THREADS) void grad_pack16_kernel(const float* __restrict__ g0, const float* __restrict__ g1, bf16_t* __restrict__ rows, int n0,
                                                                   int n1, int GP, int HW, long total) {
    const long i = (long)blockIdx.x * HEAD_THREADS + threadIdx.x;
    if (i >= total) return;
    const int G8 = GP / 8;
    const long pix = i % HW, bc = i / HW;
    const long b = bc / G8;
    const int c0 = (int)(bc - b * G8) * 8;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int col = c0 + e;
        v[e] = 0.f;
        if (col < n0) { if (g0 != nullptr) v[e] = g0[(b * n0 + col) * HW + pix]; }
        else if (col < n0 + n1) { if (g1 != nullptr) v[e] = g1[(b * n1 + (col - n0)) * HW + pix]; }
    }
    store8(rows + (b * HW + pix) * GP + c0, v);
}

// MODE 0: 1x1 (and linear); 1: 3x3, pad 1; 2: ConvTranspose2d(2, 2), stride 1 only.  A wave owns 16 outputs o x 16 CT channels c x all taps of one
// slab of the M cells of the k dimension, as kernels_detbwd.hip's wgrad_kernel does, and writes the same partial tile.  A k-step is 32 cells:
// the wave stages g (32 cells x its 16 o) and, per tap or channel tile, x (32 cells x 16 c) as images, then reads every image back as an operand:
// A = g^T (row o), B = x (column c).  MODE 2: the k dimension is the cells of x on (H, W); g lives on (2H, 2W) and is staged once per tap (dy, dx),
// the cell (2y + dy, 2x + dx) of g against the cell (y, x) of x, four channel tiles of x.  The bias gradient is the product against a column of
// ones (MODE 2: one per tap, so every row of g is counted once), taken by the waves of channel group 0.  GP: the columns of a row of g (the heads
// round c_out up to 8, the pad columns hold +0.0; the trunk: c_out).
template <int MODE, int STRIDE>
__global__ __launch_bounds__(HEAD_THREADS) void wgrad16_kernel(const cosy_head_layer_t a, const bf16_t* __restrict__ g, const int GP, const int M, const int slab,
                                                               const int n_waves, const int c_groups, const int want_db, float* __restrict__ partial,
                                                               const long slab_floats) {
    static_assert(STRIDE == 1 || (STRIDE == 2 && MODE != 2), "stride 2: 1x1 and 3x3 only");
    constexpr int TAPS = MODE == 0 ? 1 : MODE == 1 ? 9 : 4, CT = MODE == 1 ? 1 : 4;
    constexpr int GI = MODE == 2 ? 4 : 1, XI = MODE == 1 ? 9 : 4, IMAGES = GI + XI;         // images of g and of x per k-step
    __shared__ __attribute__((aligned(16))) unsigned char lds[HEAD_THREADS / 64][IMAGES * WG_IMAGE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wv = blockIdx.x * (HEAD_THREADS / 64) + wave;
    if (wv >= n_waves) return;                                 // wave-uniform: the waves that stay have EXEC all ones
    unsigned char* const img_g = lds[wave];
    unsigned char* const img_x = img_g + GI * WG_IMAGE;
    const int ot = wv / c_groups, cg = wv - ot * c_groups;
    const int j = lane & 15, kq = lane >> 4;
    const int C = a.c_in, O = a.c_out;
    const bf16_t* __restrict__ x = (const bf16_t*)a.x;
    const long k_begin = (long)blockIdx.y * slab;
    const long k_end = k_begin + slab < M ? k_begin + slab : M;
    const bool bias_wave = want_db && cg == 0;
    const int rd = WG_GROUP * kq + 32 * (j >> 2) + 8 * (j & 3);
    const int sc = lane >> 1, sh = lane & 1;                   // staging g (and a 3x3's x): the lane's cell of the step and its half of the 16 channels
    const int wr = image_off(sc) + 16 * sh;
    const bf16x8 zero = zero_frag<bf16_t>();
    bf16x8 ones;
#pragma unroll
    for (int e = 0; e < 8; ++e) ones[e] = (bf16_t)1.f;

    f32x4 acc[TAPS][CT], accb = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < TAPS; ++t)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) acc[t][ct] = f32x4{0.f, 0.f, 0.f, 0.f};

    // one k-step's rows, loaded one step ahead of their use: gv = g (this lane's cell, eight of the wave's 16 o; MODE 2: per tap), xv = x per
    // channel tile or tap
    bf16x8 gv[GI], xv[XI];
    auto load_step = [&](const long k0) {
        {
            const long cell = k0 + sc;
            const int o = ot * 16 + 8 * sh;
            const bool in = cell < k_end && o < GP;
#pragma unroll
            for (int t = 0; t < GI; ++t) gv[t] = zero;
            if constexpr (MODE != 2) {
                if (in) gv[0] = *(const bf16x8*)(g + cell * GP + o);
            } else if (in) {
                const int H = a.H[0], W = a.W[0];              // the layer's INPUT map; g lives on (2H, 2W)
                const long b = cell / ((long)H * W);
                const int pix = (int)(cell - b * H * W), py = pix / W, px = pix - py * W;
#pragma unroll
                for (int t = 0; t < GI; ++t) gv[t] = *(const bf16x8*)(g + ((b * 2 * H + 2 * py + (t >> 1)) * 2 * W + 2 * px + (t & 1)) * GP + o);
            }
        }
        if constexpr (MODE != 1) {                             // four loads: eight lanes read the 128 contiguous bytes of one cell's 64 channels
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const long cell = k0 + 8 * i + (lane >> 3);
                const int c = cg * 64 + 8 * (lane & 7);
                xv[i] = zero;
                if (cell < k_end && c < C) {
                    long xr = cell;
                    if constexpr (STRIDE == 2) {
                        const int H = a.H[0], W = a.W[0], Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
                        const long b = cell / ((long)Ho * Wo);
                        const int pix = (int)(cell - b * Ho * Wo), oy = pix / Wo;
                        xr = (b * H + 2 * oy) * W + 2 * (pix - oy * Wo);
                    }
                    xv[i] = *(const bf16x8*)(x + xr * C + c);
                }
            }
        } else {
            const long cell = k0 + sc;
            const int c = cg * 16 + 8 * sh;
            long xr = cell;
            int H = 0, W = 0, iy = 0, ix = 0;                  // H = 0: no tap is inside
            if (cell < k_end && c < C) {
                if constexpr (STRIDE == 1) {
                    int l = 0;
                    while (l + 1 < a.n_levels && cell >= a.row_start[l + 1]) ++l;
                    H = a.H[l]; W = a.W[l];
                    const int pix = (int)((cell - a.row_start[l]) % ((long)H * W));
                    iy = pix / W; ix = pix - iy * W;
                } else {
                    H = a.H[0]; W = a.W[0];
                    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
                    const long b = cell / ((long)Ho * Wo);
                    const int pix = (int)(cell - b * Ho * Wo), oy = pix / Wo;
                    iy = 2 * oy; ix = 2 * (pix - oy * Wo);
                    xr = (b * H + iy) * W + ix;
                }
            }
#pragma unroll
            for (int t = 0; t < TAPS; ++t) {
                const int dy = t / 3 - 1, dx = t - (t / 3) * 3 - 1;
                const bool tin = (unsigned)(iy + dy) < (unsigned)H && (unsigned)(ix + dx) < (unsigned)W;
                xv[t] = zero;
                if (tin) xv[t] = *(const bf16x8*)(x + (xr + dy * W + dx) * C + c);     // the address of a tap outside the map is never formed
            }
        }
    };

    if (k_begin < k_end) load_step(k_begin);
    for (long k0 = k_begin; k0 < k_end; k0 += WG_CELLS) {
#pragma unroll
        for (int t = 0; t < GI; ++t) *(bf16x8*)(img_g + t * WG_IMAGE + wr) = gv[t];
        if constexpr (MODE != 1) {
#pragma unroll
            for (int i = 0; i < 4; ++i) *(bf16x8*)(img_x + ((lane & 7) >> 1) * WG_IMAGE + image_off(8 * i + (lane >> 3)) + 16 * (lane & 1)) = xv[i];
        } else {
#pragma unroll
            for (int t = 0; t < TAPS; ++t) *(bf16x8*)(img_x + t * WG_IMAGE + wr) = xv[t];
        }
        wave_sync();
        if (k0 + WG_CELLS < k_end) load_step(k0 + WG_CELLS);  // wave-uniform; the next step's rows are in flight under this step's reads and MFMAs
        if constexpr (MODE != 2) {
            const bf16x8 af = image_frag(img_g, rd);
#pragma unroll
            for (int t = 0; t < TAPS * CT; ++t) {
                const bf16x8 bf = image_frag(img_x + t * WG_IMAGE, rd);
                if constexpr (MODE == 0) mma(acc[0][t], af, bf); else mma(acc[t][0], af, bf);
            }
            if (bias_wave) mma(accb, af, ones);                // wave-uniform
        } else {
            bf16x8 af[TAPS];
#pragma unroll
            for (int t = 0; t < TAPS; ++t) af[t] = image_frag(img_g + t * WG_IMAGE, rd);
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                const bf16x8 bf = image_frag(img_x + ct * WG_IMAGE, rd);
#pragma unroll
                for (int t = 0; t < TAPS; ++t) mma(acc[t][ct], af[t], bf);
            }
            if (bias_wave)                                     // wave-uniform; the taps ascending
#pragma unroll
                for (int t = 0; t < TAPS; ++t) mma(accb, af[t], ones);
        }
        wave_sync();
    }

    float* __restrict__ out = partial + (long)blockIdx.y * slab_floats;
    const long O16 = (long)((O + 15) / 16) * 16;
#pragma unroll
    for (int t = 0; t < TAPS; ++t)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            const int c = (cg * CT + ct) * 16 + j;
            if (c >= C) continue;
#pragma unroll
            for (int q = 0; q < 4; ++q) out[((long)(ot * 16 + 4 * kq + q) * TAPS + t) * C + c] = acc[t][ct][q];
        }
    if (cg == 0 && j == 0)                                     // without want_db the row holds zeros and nobody reads it
#pragma unroll
        for (int q = 0; q < 4; ++q) out[O16 * TAPS * C + ot * 16 + 4 * kq + q] = accb[q];
}

// the weight gradient of M cells (the k dimension) of a.c_in -> a.c_out on bfloat16 rows, after the caller's own argument checks: kernels_detbwd.hip's
// plan (slabs, workspace, M == 0) with wgrad16_kernel; outputs [0, n_split) to dw0 / db0 (db0 null: none), the rest to dw1 / db1
int run_wgrad16(const char* fn, const cosy_head_layer_t& a, int stride, long M, int GP, const bf16_t* g, const float* scale, int n_split, float* dw0, float* db0,
                float* dw1, float* db1, void* workspace, size_t workspace_bytes, hipStream_t s) {
    const int T = a.ksize == 3 ? 9 : a.ksize == 2 ? 4 : 1;
    if (M == 0) {
        const long nw0 = (long)n_split * T * a.c_in, nw1 = (long)(a.c_out - n_split) * T * a.c_in;
        COSY_CHECK_HIP(hipMemsetAsync(dw0, 0, nw0 * sizeof(float), s));
        if (db0 != nullptr) COSY_CHECK_HIP(hipMemsetAsync(db0, 0, (size_t)n_split * sizeof(float), s));
        if (nw1) {
            COSY_CHECK_HIP(hipMemsetAsync(dw1, 0, nw1 * sizeof(float), s));
            COSY_CHECK_HIP(hipMemsetAsync(db1, 0, (size_t)(a.c_out - n_split) * sizeof(float), s));
        }
        return COSY_OK;
    }
    COSY_REQUIRE(a.x != nullptr, "%s: null layer->x", fn);
    COSY_REQUIRE(g != nullptr, "%s: null g", fn);
    COSY_REQUIRE(workspace != nullptr, "%s: null workspace", fn);
    COSY_REQUIRE(((uintptr_t)a.x & 15) == 0 && ((uintptr_t)g & 15) == 0, "%s: the rows x and g must be 16-byte aligned", fn);
    const int slab = wgrad_slab_rows_of((int)M), nslab = cdiv(M, slab);
    const long slab_floats = wgrad_slab_floats_of(a.ksize, a.c_in, a.c_out);
    const size_t need = (size_t)nslab * (size_t)slab_floats * sizeof(float);
    COSY_REQUIRE(workspace_bytes >= need, "%s: workspace_bytes=%zu is less than the %zu bytes that %ld cells of c_in=%d, c_out=%d need "
                 "(cosy_head_wgrad_workspace_bytes)", fn, workspace_bytes, need, M, a.c_in, a.c_out);
    const int o_tiles = cdiv(a.c_out, 16), c_groups = cdiv(a.c_in, a.ksize == 3 ? 16 : 64);
    const long n_waves = (long)o_tiles * c_groups;
    COSY_REQUIRE(n_waves <= 0x7fffffffL, "%s: c_out=%d x c_in=%d need more than 2^31 - 1 waves", fn, a.c_out, a.c_in);
    const dim3 grid((unsigned)cdiv(n_waves, HEAD_THREADS / 64), (unsigned)nslab), block(HEAD_THREADS);
    float* partial = (float*)workspace;
    const int want_db = db0 != nullptr;
#define COSY_WGRAD16_LAUNCH(MODE, STRIDE) \
    hipLaunchKernelGGL((wgrad16_kernel<MODE, STRIDE>), grid, block, 0, s, a, g, GP, (int)M, slab, (int)n_waves, c_groups, want_db, partial, slab_floats)
    if (a.ksize == 2) COSY_WGRAD16_LAUNCH(2, 1);
    else if (a.ksize == 1 && stride == 1) COSY_WGRAD16_LAUNCH(0, 1);
    else if (a.ksize == 1) COSY_WGRAD16_LAUNCH(0, 2);
    else if (stride == 1) COSY_WGRAD16_LAUNCH(1, 1);
    else COSY_WGRAD16_LAUNCH(1, 2);
#undef COSY_WGRAD16_LAUNCH
    COSY_CHECK_HIP(hipGetLastError());
    return wgrad_combine_split(partial, nslab, slab_floats, a.ksize, a.c_in, a.c_out, n_split, scale, dw0, db0, dw1, db1, s);
}

// the one pack launch, after the caller's own argument checks: n0 (+ n1 sibling) outputs of c_in channels
int run_weight_pack16(const char* fn, const float* w0, const float* b0, const float* w1, const float* b1, const float* scale, int ksize, int c_in, int n0, int n1,
                      void* fwd, float* fwd_bias, void* bwd, hipStream_t s) {
    COSY_REQUIRE(((uintptr_t)w0 & 3) == 0 && ((uintptr_t)b0 & 3) == 0 && ((uintptr_t)w1 & 3) == 0 && ((uintptr_t)b1 & 3) == 0 && ((uintptr_t)scale & 3) == 0 &&
                 ((uintptr_t)fwd & 15) == 0 && ((uintptr_t)bwd & 15) == 0 && ((uintptr_t)fwd_bias & 3) == 0,
                 "%s: the parameters, scale and fwd_bias must be 4-byte, fwd and bwd 16-byte aligned", fn);
    const pack_sizes_t z = pack_sizes(ksize, c_in, n0, n1, pack_frag<bf16_t>::KB);
    const long total = z.n_fwd + z.n_bwd + z.n_bias;
    COSY_REQUIRE(total <= (1L << 36), "%s: %ld packed elements exceed 2^36", fn, total);
    hipLaunchKernelGGL(weight_pack16_kernel, dim3(cdiv(total, HEAD_THREADS)), dim3(HEAD_THREADS), 0, s, w0, b0, w1, b1, scale, ksize, c_in, n0, n1, (bf16_t*)fwd,
                       fwd_bias, (bf16_t*)bwd, z.n_fwd, z.n_bwd, (int)z.n_bias);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

int run_grad_pack16(const char* fn, const float* g0, const float* g1, void* rows, int B, int n0, int n1, int GP, int HW, hipStream_t s) {
    COSY_REQUIRE((long)B * HW <= HEAD_MAX_ROWS, "%s: B HW = %ld rows exceed 2^30", fn, (long)B * HW);
    if (B == 0) return COSY_OK;
    COSY_REQUIRE(rows != nullptr, "%s: null rows", fn);
    COSY_REQUIRE(((uintptr_t)rows & 15) == 0 && ((uintptr_t)g0 & 3) == 0 && ((uintptr_t)g1 & 3) == 0, "%s: rows must be 16-byte, g 4-byte aligned", fn);
    const long total = (long)B * HW * (GP / 8);
    COSY_REQUIRE(cdiv(total, HEAD_THREADS) <= 0x7fffffffL && total <= (1L << 35), "%s: %ld elements exceed 2^38", fn, total * 8);
    hipLaunchKernelGGL(grad_pack16_kernel, dim3(cdiv(total, HEAD_THREADS)), dim3(HEAD_THREADS), 0, s, g0, g1, (bf16_t*)rows, n0, n1, GP, HW, total);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

// ConvTranspose2d(2, 2): M rows of the (H / 2, W / 2) maps, the four taps of the forward GEMM (kernels_detbwd.hip's launch_deconv_dgrad on bfloat16 rows)
int launch_deconv_dgrad16(const cosy_head_layer_t& a, int M, const bf16_t* y, hipStream_t s) {
    typedef DeconvGradPolicyOf<bf16_t> P;
    const conv_grid_t c = conv_grid<bf16_t>(a, M);
    COSY_REQUIRE(c.blocks <= 0x7fffffffL, "cosy_head_dgrad16: %d rows x c_out=%d need more than 2^31 - 1 workgroups", M, a.c_out);
    const dim3 grid((unsigned)c.blocks), block(HEAD_THREADS);
    const grad_epi_of<bf16_t> e{y};
    if (c.big_m && c.big_n) hipLaunchKernelGGL((conv_gemm_kernel<bf16_t, TILE_MT_BIG, TILE_NT_BIG, P>), grid, block, 0, s, a, M, c.KBn, c.n_tiles, c.n_groups, e);
    else if (c.big_m) hipLaunchKernelGGL((conv_gemm_kernel<bf16_t, TILE_MT_BIG, 1, P>), grid, block, 0, s, a, M, c.KBn, c.n_tiles, c.n_groups, e);
    else if (c.big_n) hipLaunchKernelGGL((conv_gemm_kernel<bf16_t, 1, TILE_NT_BIG, P>), grid, block, 0, s, a, M, c.KBn, c.n_tiles, c.n_groups, e);
    else hipLaunchKernelGGL((conv_gemm_kernel<bf16_t, 1, 1, P>), grid, block, 0, s, a, M, c.KBn, c.n_tiles, c.n_groups, e);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

inline int pad8(int n) { return (n + 7) / 8 * 8; }

#define COSY_REQUIRE_BF16(fn, dtype, other) \
    COSY_REQUIRE((dtype) == COSY_BF16, fn ": dtype=%d is not COSY_BF16 (float32 rows: " other "; float16 training needs a loss scaler, which is not built)", (dtype))

}  // namespace
}  // namespace cosy

using namespace cosy;

extern "C" {

int cosy_trunk_weight_pack16(const float* w, const float* scale, const float* shift, int ksize, int c_in, int c_out, void* fwd, float* fwd_bias, void* bwd,
                             cosy_stream_t stream) {
    COSY_REQUIRE(ksize == 1 || ksize == 3, "cosy_trunk_weight_pack16: ksize=%d must be 1 or 3", ksize);
    COSY_REQUIRE(c_in >= 8 && c_in % 8 == 0 && c_in <= (1 << 24), "cosy_trunk_weight_pack16: c_in=%d must be a positive multiple of 8", c_in);
    COSY_REQUIRE(c_out >= 8 && c_out % 8 == 0 && c_out <= (1 << 22), "cosy_trunk_weight_pack16: c_out=%d must be a positive multiple of 8", c_out);
    COSY_REQUIRE_PTR("cosy_trunk_weight_pack16", w); COSY_REQUIRE_PTR("cosy_trunk_weight_pack16", shift);
    COSY_REQUIRE_PTR("cosy_trunk_weight_pack16", fwd); COSY_REQUIRE_PTR("cosy_trunk_weight_pack16", fwd_bias); COSY_REQUIRE_PTR("cosy_trunk_weight_pack16", bwd);
    return run_weight_pack16("cosy_trunk_weight_pack16", w, shift, nullptr, nullptr, scale, ksize, c_in, c_out, 0, fwd, fwd_bias, bwd, (hipStream_t)stream);
}

int cosy_trunk_grad_pack16(const float* g, void* rows, int B, int C, int HW, cosy_stream_t stream) {
    COSY_REQUIRE(B >= 0 && HW >= 1, "cosy_trunk_grad_pack16: B=%d must be >= 0 and HW=%d >= 1", B, HW);
    COSY_REQUIRE(C >= 8 && C % 8 == 0 && C <= (1 << 20), "cosy_trunk_grad_pack16: C=%d must be a positive multiple of 8", C);
    return run_grad_pack16("cosy_trunk_grad_pack16", g, nullptr, rows, B, C, 0, C, HW, (hipStream_t)stream);
}

int cosy_head_weight_pack16(const float* w0, const float* b0, const float* w1, const float* b1, int ksize, int c_in, int n0, int n1, void* fwd, float* fwd_bias,
                            void* bwd, cosy_stream_t stream) {
    COSY_REQUIRE(ksize == 1 || ksize == 2 || ksize == 3, "cosy_head_weight_pack16: ksize=%d must be 1, 3 or 2 (ConvTranspose2d(2, 2))", ksize);
    COSY_REQUIRE(c_in >= 8 && c_in % 8 == 0 && c_in <= (1 << 24), "cosy_head_weight_pack16: the reduction length c_in=%d must be a positive multiple of 8", c_in);
    COSY_REQUIRE(n0 >= 1 && n1 >= 0 && (long)n0 + n1 <= (1 << 22), "cosy_head_weight_pack16: n0=%d must be >= 1 and n1=%d >= 0", n0, n1);
    COSY_REQUIRE(ksize != 2 || (n1 == 0 && n0 % 8 == 0), "cosy_head_weight_pack16: a deconvolution has no sibling and n0=%d a multiple of 8", n0);
    COSY_REQUIRE_PTR("cosy_head_weight_pack16", w0); COSY_REQUIRE_PTR("cosy_head_weight_pack16", b0);
    COSY_REQUIRE_PTR("cosy_head_weight_pack16", fwd); COSY_REQUIRE_PTR("cosy_head_weight_pack16", fwd_bias); COSY_REQUIRE_PTR("cosy_head_weight_pack16", bwd);
    COSY_REQUIRE(n1 == 0 || (w1 != nullptr && b1 != nullptr), "cosy_head_weight_pack16: null w1 or b1 with n1=%d", n1);
    return run_weight_pack16("cosy_head_weight_pack16", w0, b0, w1, b1, nullptr, ksize, c_in, n0, n1, fwd, fwd_bias, bwd, (hipStream_t)stream);
}

int cosy_head_grad_pack16(const float* g0, const float* g1, void* rows, int B, int n0, int n1, int HW, cosy_stream_t stream) {
    COSY_REQUIRE(B >= 0 && HW >= 1, "cosy_head_grad_pack16: B=%d must be >= 0 and HW=%d >= 1", B, HW);
    COSY_REQUIRE(n0 >= 0 && n1 >= 0 && n0 + n1 >= 1 && n0 + n1 <= (1 << 20), "cosy_head_grad_pack16: n0=%d and n1=%d must be >= 0 and hold 1 to 2^20 columns", n0, n1);
    return run_grad_pack16("cosy_head_grad_pack16", g0, g1, rows, B, n0, n1, pad8(n0 + n1), HW, (hipStream_t)stream);
}

int cosy_head_dgrad16(const cosy_head_layer_t* layer, const void* y, cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    COSY_REQUIRE_PTR("cosy_head_dgrad16", layer);
    const cosy_head_layer_t& a = *layer;
    COSY_REQUIRE_BF16("cosy_head_dgrad16", a.dtype, "cosy_head_dgrad");
    COSY_REQUIRE(a.ksize == 1 || a.ksize == 2 || a.ksize == 3, "cosy_head_dgrad16: ksize=%d must be 1, 3 or 2 (ConvTranspose2d(2, 2))", a.ksize);
    COSY_REQUIRE(a.c_in >= 8 && a.c_in % 8 == 0, "cosy_head_dgrad16: the reduction length c_in=%d must be a positive multiple of 8", a.c_in);
    COSY_REQUIRE(a.c_out >= 8 && a.c_out % 8 == 0, "cosy_head_dgrad16: c_out=%d (the layer's input channels) must be a positive multiple of 8", a.c_out);
    COSY_REQUIRE(a.store == COSY_HEAD_STORE_ROWS || a.store == COSY_HEAD_STORE_NCHW, "cosy_head_dgrad16: store=%d is not COSY_HEAD_STORE_ROWS or COSY_HEAD_STORE_NCHW", a.store);
    COSY_REQUIRE(a.relu == 0, "cosy_head_dgrad16: relu=%d must be 0 (the mask is given by y)", a.relu);
    COSY_REQUIRE(a.store != COSY_HEAD_STORE_NCHW || (a.n_split == a.c_out && y == nullptr), "cosy_head_dgrad16: an NCHW store takes n_split == c_out=%d and no y", a.c_out);
    const long rows_in = check_levels("cosy_head_dgrad16", a);
    if (rows_in < 0) return COSY_EINVAL;
    long M = rows_in;
    if (a.ksize == 2) {
        COSY_REQUIRE(a.n_levels == 1 && a.H[0] % 2 == 0 && a.W[0] % 2 == 0, "cosy_head_dgrad16: ksize 2 takes one level of even maps, got %d levels of %d x %d",
                     a.n_levels, a.H[0], a.W[0]);
        M = rows_in / 4;
    }
    if (M == 0) return COSY_OK;
    COSY_REQUIRE_PTR("cosy_head_dgrad16", a.x); COSY_REQUIRE_PTR("cosy_head_dgrad16", a.w); COSY_REQUIRE_PTR("cosy_head_dgrad16", a.out);
    COSY_REQUIRE(((uintptr_t)a.x & 15) == 0 && ((uintptr_t)a.w & 15) == 0 && ((uintptr_t)a.out & 15) == 0 && ((uintptr_t)y & 15) == 0,
                 "cosy_head_dgrad16: x, w, out and y must be 16-byte aligned");
    if (a.ksize == 2) return launch_deconv_dgrad16(a, (int)M, (const bf16_t*)y, s);
    const tadd_t<bf16_t> none{nullptr, ADD_NONE, 1, 1, 1.f, 1.f};
    return launch_dgrad_rows<bf16_t, 1>("cosy_head_dgrad16", a, (int)M, tgrad_epi_t<bf16_t>{(const bf16_t*)y, {none, none}, 0, 0}, s);
}

int cosy_head_wgrad16(const cosy_head_layer_t* layer, const void* g, float* dw0, float* db0, float* dw1, float* db1, void* workspace, size_t workspace_bytes,
                      cosy_stream_t stream) {
    COSY_REQUIRE_PTR("cosy_head_wgrad16", layer);
    const cosy_head_layer_t& a = *layer;
    COSY_REQUIRE_BF16("cosy_head_wgrad16", a.dtype, "cosy_head_wgrad");
    COSY_REQUIRE(a.ksize == 1 || a.ksize == 2 || a.ksize == 3, "cosy_head_wgrad16: ksize=%d must be 1, 3 or 2 (ConvTranspose2d(2, 2))", a.ksize);
    COSY_REQUIRE(a.c_in >= 8 && a.c_in % 8 == 0, "cosy_head_wgrad16: c_in=%d must be a positive multiple of 8", a.c_in);
    COSY_REQUIRE(a.c_out >= 1 && a.c_out <= (1 << 22), "cosy_head_wgrad16: c_out=%d must lie in [1, 2^22]", a.c_out);
    COSY_REQUIRE(a.n_split >= 1 && a.n_split <= a.c_out, "cosy_head_wgrad16: n_split=%d must lie in [1, c_out=%d]", a.n_split, a.c_out);
    COSY_REQUIRE(a.ksize != 2 || (a.n_levels == 1 && a.n_split == a.c_out && a.c_out % 8 == 0),
                 "cosy_head_wgrad16: ksize 2 takes one level, no sibling and c_out=%d a multiple of 8", a.c_out);
    const long M = check_levels("cosy_head_wgrad16", a);
    if (M < 0) return COSY_EINVAL;
    COSY_REQUIRE(a.ksize != 2 || 4 * M <= HEAD_MAX_ROWS, "cosy_head_wgrad16: 4 x %ld gradient rows exceed 2^30", M);
    COSY_REQUIRE_PTR("cosy_head_wgrad16", dw0); COSY_REQUIRE_PTR("cosy_head_wgrad16", db0);
    COSY_REQUIRE(a.n_split == a.c_out || (dw1 != nullptr && db1 != nullptr), "cosy_head_wgrad16: null dw1 or db1 with n_split=%d < c_out=%d", a.n_split, a.c_out);
    COSY_REQUIRE(((uintptr_t)dw0 & 3) == 0 && ((uintptr_t)db0 & 3) == 0 && ((uintptr_t)dw1 & 3) == 0 && ((uintptr_t)db1 & 3) == 0 && ((uintptr_t)workspace & 3) == 0,
                 "cosy_head_wgrad16: dw0, db0, dw1, db1 and workspace must be 4-byte aligned");
    const int T = a.ksize == 3 ? 9 : a.ksize == 2 ? 4 : 1;
    COSY_REQUIRE((long)a.c_out * T * a.c_in + a.c_out <= (1L << 36), "cosy_head_wgrad16: c_out=%d x c_in=%d weights exceed 2^36", a.c_out, a.c_in);
    return run_wgrad16("cosy_head_wgrad16", a, 1, M, pad8(a.c_out), (const bf16_t*)g, nullptr, a.n_split, dw0, db0, dw1, db1, workspace, workspace_bytes,
                       (hipStream_t)stream);
}

int cosy_trunk_dgrad16(const cosy_head_layer_t* layer, int stride, const void* add0, int rule0, int add0_H, int add0_W, const void* add1, int rule1, int add1_H,
                       int add1_W, const void* y, cosy_stream_t stream) {
    COSY_REQUIRE_PTR("cosy_trunk_dgrad16", layer);
    COSY_REQUIRE(layer->dtype == COSY_BF16, "cosy_trunk_dgrad16: dtype=%d is not COSY_BF16 (float32 rows: cosy_trunk_dgrad; float16 training needs a loss scaler, "
                 "which is not built)", layer->dtype);
    return run_trunk_dgrad<bf16_t>("cosy_trunk_dgrad16", *layer, stride, (const bf16_t*)add0, rule0, add0_H, add0_W, (const bf16_t*)add1, rule1, add1_H, add1_W,
                                   (const bf16_t*)y, (hipStream_t)stream);
}

int cosy_trunk_wgrad16(const cosy_head_layer_t* layer, int stride, const void* g, const float* scale, float* dw, float* db, void* workspace, size_t workspace_bytes,
                       cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    COSY_REQUIRE_PTR("cosy_trunk_wgrad16", layer);
    const cosy_head_layer_t& a = *layer;
    COSY_REQUIRE(a.dtype == COSY_BF16, "cosy_trunk_wgrad16: dtype=%d is not COSY_BF16 (float32 rows: cosy_trunk_wgrad; float16 training needs a loss scaler, which is "
                 "not built)", a.dtype);
    COSY_REQUIRE(a.ksize == 1 || a.ksize == 3, "cosy_trunk_wgrad16: ksize=%d must be 1 or 3", a.ksize);
    COSY_REQUIRE(stride == 1 || stride == 2, "cosy_trunk_wgrad16: stride=%d must be 1 or 2", stride);
    COSY_REQUIRE(a.c_in >= 8 && a.c_in % 8 == 0, "cosy_trunk_wgrad16: c_in=%d must be a positive multiple of 8", a.c_in);
    COSY_REQUIRE(a.c_out >= 8 && a.c_out % 8 == 0 && a.c_out <= (1 << 22), "cosy_trunk_wgrad16: c_out=%d must be a positive multiple of 8", a.c_out);
    const long M_in = check_levels("cosy_trunk_wgrad16", a);
    if (M_in < 0) return COSY_EINVAL;
    COSY_REQUIRE(stride == 1 || a.n_levels == 1, "cosy_trunk_wgrad16: stride=2 takes one level, got n_levels=%d", a.n_levels);
    const int Ho = (a.H[0] - 1) / stride + 1, Wo = (a.W[0] - 1) / stride + 1;
    const long M = stride == 1 ? M_in : M_in / ((long)a.H[0] * a.W[0]) * Ho * Wo;       // the OUTPUT cells: the k dimension
    COSY_REQUIRE_PTR("cosy_trunk_wgrad16", dw);
    COSY_REQUIRE(((uintptr_t)dw & 3) == 0 && ((uintptr_t)db & 3) == 0 && ((uintptr_t)scale & 3) == 0 && ((uintptr_t)workspace & 3) == 0,
                 "cosy_trunk_wgrad16: scale, dw, db and workspace must be 4-byte aligned");
    COSY_REQUIRE((long)a.c_out * (a.ksize == 3 ? 9 : 1) * a.c_in <= (1L << 36), "cosy_trunk_wgrad16: c_out=%d x c_in=%d weights exceed 2^36", a.c_out, a.c_in);
    return run_wgrad16("cosy_trunk_wgrad16", a, stride, M, a.c_out, (const bf16_t*)g, scale, a.c_out, dw, db, nullptr, nullptr, workspace, workspace_bytes, s);
}

}  // extern "C"
