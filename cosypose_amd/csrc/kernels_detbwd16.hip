// The weight gradient of the detector's trunk and heads (section 32) on bfloat16 rows: the first pass of kernels_detbwd.hip's
// run_wgrad<bf16_t>.  Every other kernel of the bfloat16 backward, the plan and every entry point are in kernels_detbwd.hip and detbwd_device.h,
// one text for both row types.
//   * wgrad16_kernel: dW[o][tap][c] = sum over OUTPUT cells of g[cell][o] x[cell + tap][c] with the CELLS as the k dimension of
//     v_mfma_f32_16x16x32_bf16.  The instruction wants eight consecutive cells of ONE channel per lane for both operands; the rows are stored
//     cell-major.  A wave loads whole row segments (16 bytes: eight channels of one cell per lane), lays 32 cells x 16 channels images in LDS and
//     reads them back transposed with ds_read_b64_tr_b16.  The image: a cell's 16 channels are 32 contiguous bytes, eight cells a 256-byte group,
//     and every group is followed by 128 bytes of pad (group stride 384).  One transposed read of a 32-lane half takes cells 8 G .. 8 G + 3 of
//     two neighbouring groups G: 2 x 128 contiguous bytes that start 384 bytes apart, i.e. banks [0, 32) and [32, 64) (or the reverse): all 64
//     banks once, no conflict by the bank rule.  Every wave owns its images: no barrier, only wave-level ordering of its own LDS traffic, and
//     EXEC is all ones at every transposed read (a wave past the last tile leaves as a whole; cells past the slab, taps outside the map and
//     channels past the row are staged as +0.0, never masked).
//     Slabs, workspace, partial tiles, the ascending second pass and the one scale[o] product are kernels_detbwd.hip's.
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

}  // namespace

// the bfloat16 rows' first pass; the float32 rows' is kernels_detbwd.hip's
void detbwd::launch_wgrad(const cosy_head_layer_t& a, int stride, const bf16_t* g, const wgrad_plan_t& p, hipStream_t s) {
    const dim3 grid((unsigned)cdiv(p.n_waves, HEAD_THREADS / 64), (unsigned)p.nslab), block(HEAD_THREADS);
#define COSY_WGRAD16_LAUNCH(MODE, STRIDE) \
    hipLaunchKernelGGL((wgrad16_kernel<MODE, STRIDE>), grid, block, 0, s, a, g, p.GP, p.M, p.slab, p.n_waves, p.c_groups, p.want_db, p.partial, p.slab_floats)
    if (a.ksize == 2) COSY_WGRAD16_LAUNCH(2, 1);
    else if (a.ksize == 1 && stride == 1) COSY_WGRAD16_LAUNCH(0, 1);
    else if (a.ksize == 1) COSY_WGRAD16_LAUNCH(0, 2);
    else if (stride == 1) COSY_WGRAD16_LAUNCH(1, 1);
    else COSY_WGRAD16_LAUNCH(1, 2);
#undef COSY_WGRAD16_LAUNCH
}

}  // namespace cosy
