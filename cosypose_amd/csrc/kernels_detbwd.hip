// The backward of the detector on the matrix pipe, float32 only: the heads and the trunk (section 29) run ONE set of
// gradient kernels.  A layer is v = conv_stride(x, W) [scale + shift] [+ r], y = act(v) (kernels_dethead.hip, kernels_dettrunk.hip); g is the
// gradient at v, float32 rows on the layer's OUTPUT grid (heads: c_out rounded up to 8, the pad +0.0).
//   * data gradient   dX[cell][c] = sum over (tap, o) of w[o][tap][c] g[cell - tap][o]: detbwd_device.h's dgrad_rows_kernel<float>, the forward GEMM's chain (dethead_device.h:
//     accumulator +0.0, blocks of 16 o ascending, the taps of the flipped packing ascending inside a block, every term one fmaf) over the rows g
//     with the weight transposed and its taps flipped.  At stride 2 a launch owns ONE parity class of (iy, ix) and runs only that class's live
//     taps (1, 2, 2 or 4 of 9).  Its store adds up to two operands (SAME, EVEN, NEAREST_T: the trunk's shortcuts and the FPN), applies the ReLU
//     mask of the layer below and writes rows or NCHW, so the launch writes that layer's pre-activation gradient.  ConvTranspose2d(2, 2) alone
//     stays on conv_gemm_kernel (DeconvGradPolicy): its four stride-2 taps over the rows of the (2H, 2W) map.
//   * weight gradient dW[o][tap][c] = [scale[o]] sum over OUTPUT cells of g[(y, x)][o] x[(stride y + dy, stride x + dx)][c], bias gradient
//     db[o] = sum over cells of g[cell][o]: wgrad_kernel, v_mfma_f32_16x16x4_f32 with the CELLS as the k dimension, streamed once.  The cells are
//     cut into slabs (cosy_head_wgrad_slab_rows); a wave writes its slab's partial tile, wgrad_combine_kernel adds the slabs in ascending order,
//     multiplies by scale[o] once and writes torchvision's layout.  No atomics: two calls give equal bits.
//   * grad_pack_kernel makes the rows g out of the losses' NCHW gradients; weight_pack_kernel makes both fragment-order weights (forward, and
//     transposed + flipped [x scale[o], rounded once] for the data gradient) out of a parameter in torchvision's layout, on the device.
// No atomics, no LDS: equal inputs give equal bits.
#include "detbwd_device.h"

namespace cosy {
namespace {

using namespace headgemm;
using namespace detbwd;                      // the data gradient: kernel, store rules and entry checks, one template over the type of the rows

constexpr int WG_SLAB_MIN = 256;             // cells of a slab: at least this many, and at most WG_MAX_SLABS slabs
constexpr int WG_MAX_SLABS = 16;

inline int pad8(int n) { return (n + 7) / 8 * 8; }
inline int wgrad_slab_rows(int M) {
    const long per = ((long)M + WG_MAX_SLABS - 1) / WG_MAX_SLABS;
    const long s = (per + 3) / 4 * 4;
    return (int)(s > WG_SLAB_MIN ? s : WG_SLAB_MIN);
}
// floats of one slab's partial: [c_out rounded up to 16][taps][c_in], then the bias row
inline long wgrad_slab_floats(int ksize, int c_in, int c_out) {
    const long O16 = (c_out + 15) / 16 * 16, taps = ksize == 3 ? 9 : ksize == 2 ? 4 : 1;
    return O16 * taps * c_in + O16;
}

// NCHW float32 (B, n0, HW) and (B, n1, HW) -> rows (B HW, GP): the columns of the first, then of the second, then +0.0.  A null tensor is zeros.
__global__ __launch_bounds__(HEAD_THREADS) void head_grad_pack_kernel(const float* __restrict__ g0, const float* __restrict__ g1, float* __restrict__ rows,
                                                                      int n0, int n1, int GP, int HW, long total) {
    const long i = (long)blockIdx.x * HEAD_THREADS + threadIdx.x;
    if (i >= total) return;
    const long row = i / GP;
    const int col = (int)(i - row * GP);
    const long b = row / HW, pix = row - b * HW;
    float v = 0.f;
    if (col < n0) { if (g0 != nullptr) v = g0[(b * n0 + col) * HW + pix]; }
    else if (col < n0 + n1) { if (g1 != nullptr) v = g1[(b * n1 + (col - n0)) * HW + pix]; }
    rows[i] = v;
}

// cosy_head_weight_pack / cosy_trunk_weight_pack: one thread per element of [fwd | bwd | fwd_bias]; the rules are detbwd_device.h's weight_pack_element
// (float32: 16 of the reduction per block, four elements per lane)
__global__ __launch_bounds__(HEAD_THREADS) void weight_pack_kernel(const float* __restrict__ w0, const float* __restrict__ b0, const float* __restrict__ w1,
                                                                   const float* __restrict__ b1, const float* __restrict__ scale, int ksize, int C, int n0, int n1,
                                                                   float* __restrict__ fwd, float* __restrict__ fwd_bias, float* __restrict__ bwd, long n_fwd,
                                                                   long n_bwd, int n_bias) {
    weight_pack_element<float>((long)blockIdx.x * HEAD_THREADS + threadIdx.x, w0, b0, w1, b1, scale, ksize, C, n0, n1, fwd, fwd_bias, bwd, n_fwd, n_bwd, n_bias);
}

// MODE 0: one tap (1x1 conv, linear); 1: 3x3, pad 1; 2: ConvTranspose2d(2, 2), stride 1 only.  A wave owns 16 outputs o x 16 CT channels c x all
// taps of one slab of the M OUTPUT cells: the cell (y, x) of g meets the cell (stride y + dy, stride x + dx) of x.  a.H / a.W / a.row_start: the
// maps of x; stride 2: one level.  The MFMA's A operand is g^T (row o = lane & 15, k = the cell lane >> 4), its B operand x (k = the cell, column
// c = lane & 15), four cells per instruction; the result has o = 4 (lane >> 4) + reg, c = lane & 15.  The bias gradient (want_db) is the same
// product against a column of ones, taken by the waves of channel group 0 last in a k-step.  A cell past the slab, a tap outside the map and a
// column past the row feed +0.0; no address is formed.  GP: the columns of a row of g.  STRIDE is a template parameter: as a kernel argument it
// cost the heads' 3x3 layers 3 % of their weight gradient's time (the loop then holds both branches of the address).
template <int MODE, int STRIDE>
__global__ __launch_bounds__(HEAD_THREADS) void wgrad_kernel(const cosy_head_layer_t a, const float* __restrict__ g, const int GP, const int M, const int slab,
                                                             const int n_waves, const int c_groups, const int want_db, float* __restrict__ partial,
                                                             const long slab_floats) {
    static_assert(STRIDE == 1 || (STRIDE == 2 && MODE != 2), "stride 2: 1x1 and 3x3 only");
    constexpr int TAPS = MODE == 0 ? 1 : MODE == 1 ? 9 : 4, CT = MODE == 0 ? 4 : 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wv = blockIdx.x * (HEAD_THREADS / 64) + wave;
    if (wv >= n_waves) return;                                 // wave-uniform
    const int ot = wv / c_groups, cg = wv - ot * c_groups;
    const int j = lane & 15, kq = lane >> 4;
    const int C = a.c_in;
    const float* __restrict__ x = (const float*)a.x;
    const long k_begin = (long)blockIdx.y * slab;
    const long k_end = k_begin + slab < M ? k_begin + slab : M;
    const int o_a = ot * 16 + j;                               // the A operand's output column of g
    const bool o_in = o_a < GP;
    const bool bias_wave = want_db && cg == 0;

    f32x4 acc[TAPS][CT], accb = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < TAPS; ++t)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) acc[t][ct] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (long k0 = k_begin; k0 < k_end; k0 += 4) {
        const long cell = k0 + kq;
        const bool in = cell < k_end;
        if constexpr (MODE == 2) {
            const int c = cg * 16 + j;
            const float bv = in && c < C ? x[cell * C + c] : 0.f;
            float av[TAPS] = {0.f, 0.f, 0.f, 0.f};
            if (in && o_in) {
                const int H = a.H[0], W = a.W[0];              // the layer's INPUT map; g lives on (2H, 2W)
                const long b = cell / ((long)H * W);
                const int pix = (int)(cell - b * H * W), py = pix / W, px = pix - py * W;
#pragma unroll
                for (int t = 0; t < TAPS; ++t) av[t] = g[((b * 2 * H + 2 * py + (t >> 1)) * 2 * W + 2 * px + (t & 1)) * GP + o_a];
            }
#pragma unroll
            for (int t = 0; t < TAPS; ++t) acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t], bv, acc[t][0], 0, 0, 0);
            if (bias_wave)
#pragma unroll
                for (int t = 0; t < TAPS; ++t) accb = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t], 1.f, accb, 0, 0, 0);
        } else {
            const float av = in && o_in ? g[cell * GP + o_a] : 0.f;
            // the row of x under the centre tap, and its map and place for the border test (a 1x1 at stride 1 needs neither: the row is the cell)
            const bool live = in && (MODE == 0 || cg * 16 + j < C);
            long xr = cell;
            int H = 0, W = 0, iy = 0, ix = 0;                  // H = 0: no tap is inside
            if (live && (MODE == 1 || STRIDE != 1)) {
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
            if constexpr (MODE == 0) {
                float bv[CT];
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) {
                    const int c = (cg * CT + ct) * 16 + j;
                    bv[ct] = live && c < C ? x[xr * C + c] : 0.f;
                }
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) acc[0][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[ct], acc[0][ct], 0, 0, 0);
            } else {
                const int c = cg * 16 + j;
                float bv[TAPS];
#pragma unroll
                for (int t = 0; t < TAPS; ++t) {
                    const int dy = t / 3 - 1, dx = t - (t / 3) * 3 - 1;
                    const bool tin = (unsigned)(iy + dy) < (unsigned)H && (unsigned)(ix + dx) < (unsigned)W;
                    bv[t] = tin ? x[(xr + dy * W + dx) * C + c] : 0.f;
                }
#pragma unroll
                for (int t = 0; t < TAPS; ++t) acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[t], acc[t][0], 0, 0, 0);
            }
            if (bias_wave) accb = __builtin_amdgcn_mfma_f32_16x16x4f32(av, 1.f, accb, 0, 0, 0);
        }
    }

    float* __restrict__ out = partial + (long)blockIdx.y * slab_floats;
    const long O16 = (long)((a.c_out + 15) / 16) * 16;
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

// slab 0, then + slab 1, + slab 2, ...; then ONE rounded product with scale[o] (null: none; db has no scale); one thread per element of the
// results, which it writes in torchvision's layout: ksize 1 / 3: (O, C, k, k), outputs [0, n_split) to dw0 / db0 and the rest to dw1 / db1;
// ksize 2: (C, O, 2, 2).  db0 null: no bias gradient is written
__global__ __launch_bounds__(HEAD_THREADS) void wgrad_combine_kernel(const float* __restrict__ partial, int nslab, long slab_floats, int ksize, int C, int O,
                                                                     int n_split, const float* __restrict__ scale, float* __restrict__ dw0,
                                                                     float* __restrict__ db0, float* __restrict__ dw1, float* __restrict__ db1) {
    const int T = ksize == 3 ? 9 : ksize == 2 ? 4 : 1;
    const long n_w = (long)O * T * C, O16 = (long)((O + 15) / 16) * 16;
    const long i = (long)blockIdx.x * HEAD_THREADS + threadIdx.x;
    if (i >= n_w + (db0 != nullptr ? O : 0)) return;
    const long src = i < n_w ? i : O16 * T * C + (i - n_w);
    float acc = partial[src];
    for (int s = 1; s < nslab; ++s) acc = acc + partial[(long)s * slab_floats + src];
    if (i >= n_w) {
        const int o = (int)(i - n_w);
        if (o < n_split) db0[o] = acc; else db1[o - n_split] = acc;
        return;
    }
    const int o = (int)(i / ((long)T * C)), t = (int)((i / C) % T), c = (int)(i % C);
    if (scale != nullptr) acc = acc * scale[o];
    if (ksize == 2) dw0[((long)c * O + o) * 4 + t] = acc;
    else if (o < n_split) dw0[((long)o * C + c) * T + t] = acc;
    else dw1[((long)(o - n_split) * C + c) * T + t] = acc;
}

// ConvTranspose2d(2, 2): M rows of the (H / 2, W / 2) maps, the four taps of the forward GEMM
int launch_deconv_dgrad(const cosy_head_layer_t& a, int M, const float* y, hipStream_t s) {
    const conv_grid_t c = conv_grid<float>(a, M);
    COSY_REQUIRE(c.blocks <= 0x7fffffffL, "cosy_head_dgrad: %d rows x c_out=%d need more than 2^31 - 1 workgroups", M, a.c_out);
    const dim3 grid((unsigned)c.blocks), block(HEAD_THREADS);
    const grad_epi_t e{y};
    if (c.big_m && c.big_n) hipLaunchKernelGGL((conv_gemm_kernel<float, TILE_MT_BIG, TILE_NT_BIG, DeconvGradPolicy>), grid, block, 0, s, a, M, c.KBn, c.n_tiles, c.n_groups, e);
    else if (c.big_m) hipLaunchKernelGGL((conv_gemm_kernel<float, TILE_MT_BIG, 1, DeconvGradPolicy>), grid, block, 0, s, a, M, c.KBn, c.n_tiles, c.n_groups, e);
    else if (c.big_n) hipLaunchKernelGGL((conv_gemm_kernel<float, 1, TILE_NT_BIG, DeconvGradPolicy>), grid, block, 0, s, a, M, c.KBn, c.n_tiles, c.n_groups, e);
    else hipLaunchKernelGGL((conv_gemm_kernel<float, 1, 1, DeconvGradPolicy>), grid, block, 0, s, a, M, c.KBn, c.n_tiles, c.n_groups, e);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

// One weight gradient, planned and launched, after the caller's own argument checks: M OUTPUT cells (the k dimension) of a layer a.c_in ->
// a.c_out at `stride`; outputs [0, n_split) go to dw0 / db0 (db0 null: no bias gradient), the rest to dw1 / db1.  M == 0: zeros of the right shape.
int run_wgrad(const char* fn, const cosy_head_layer_t& a, int stride, long M, const float* g, const float* scale, int n_split, float* dw0, float* db0, float* dw1,
              float* db1, void* workspace, size_t workspace_bytes, hipStream_t s) {
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
    COSY_REQUIRE(a.x != nullptr, "%s: null a.x", fn);
    COSY_REQUIRE(g != nullptr, "%s: null g", fn);
    COSY_REQUIRE(workspace != nullptr, "%s: null workspace", fn);
    const int slab = wgrad_slab_rows((int)M), nslab = cdiv(M, slab);
    const long slab_floats = wgrad_slab_floats(a.ksize, a.c_in, a.c_out);
    const size_t need = (size_t)nslab * (size_t)slab_floats * sizeof(float);
    COSY_REQUIRE(workspace_bytes >= need, "%s: workspace_bytes=%zu is less than the %zu bytes that %ld cells of c_in=%d, c_out=%d need "
                 "(cosy_head_wgrad_workspace_bytes)", fn, workspace_bytes, need, M, a.c_in, a.c_out);
    const int GP = a.ksize == 2 ? a.c_out : pad8(a.c_out);
    const int o_tiles = cdiv(a.c_out, 16), c_groups = cdiv(a.c_in, a.ksize == 1 ? 64 : 16);
    const long n_waves = (long)o_tiles * c_groups;
    COSY_REQUIRE(n_waves <= 0x7fffffffL, "%s: c_out=%d x c_in=%d need more than 2^31 - 1 waves", fn, a.c_out, a.c_in);
    const dim3 grid((unsigned)cdiv(n_waves, HEAD_THREADS / 64), (unsigned)nslab), block(HEAD_THREADS);
    float* partial = (float*)workspace;
    const int want_db = db0 != nullptr;
#define COSY_WGRAD_LAUNCH(MODE, STRIDE) \
    hipLaunchKernelGGL((wgrad_kernel<MODE, STRIDE>), grid, block, 0, s, a, g, GP, (int)M, slab, (int)n_waves, c_groups, want_db, partial, slab_floats)
    if (a.ksize == 2) COSY_WGRAD_LAUNCH(2, 1);
    else if (a.ksize == 1 && stride == 1) COSY_WGRAD_LAUNCH(0, 1);
    else if (a.ksize == 1) COSY_WGRAD_LAUNCH(0, 2);
    else if (stride == 1) COSY_WGRAD_LAUNCH(1, 1);
    else COSY_WGRAD_LAUNCH(1, 2);
#undef COSY_WGRAD_LAUNCH
    COSY_CHECK_HIP(hipGetLastError());
    const long n_out = (long)a.c_out * T * a.c_in + a.c_out;
    hipLaunchKernelGGL(wgrad_combine_kernel, dim3(cdiv(n_out, HEAD_THREADS)), block, 0, s, partial, nslab, slab_floats, a.ksize, a.c_in, a.c_out, n_split, scale,
                       dw0, db0, dw1, db1);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

// the one pack launch, after the caller's own argument checks: n0 (+ n1 sibling) outputs of c_in channels
int run_weight_pack(const char* fn, const float* w0, const float* b0, const float* w1, const float* b1, const float* scale, int ksize, int c_in, int n0, int n1,
                    float* fwd, float* fwd_bias, float* bwd, hipStream_t s) {
    const pack_sizes_t z = pack_sizes(ksize, c_in, n0, n1, pack_frag<float>::KB);
    const long total = z.n_fwd + z.n_bwd + z.n_bias;
    COSY_REQUIRE(total <= (1L << 36), "%s: %ld packed elements exceed 2^36", fn, total);
    hipLaunchKernelGGL(weight_pack_kernel, dim3(cdiv(total, HEAD_THREADS)), dim3(HEAD_THREADS), 0, s, w0, b0, w1, b1, scale, ksize, c_in, n0, n1, fwd, fwd_bias, bwd,
                       z.n_fwd, z.n_bwd, (int)z.n_bias);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

}  // namespace

// The slab rule and the second pass do not depend on the type of the rows: kernels_detbwd16.hip (section 30) reaches them here (host code only;
// declared in detbwd_device.h).  wgrad_combine: one scale, no sibling, the trunk's form; wgrad_combine_split: the heads'.
namespace detbwd {
int wgrad_slab_rows_of(int M) { return wgrad_slab_rows(M); }
long wgrad_slab_floats_of(int ksize, int c_in, int c_out) { return wgrad_slab_floats(ksize, c_in, c_out); }
int wgrad_combine_split(const float* partial, int nslab, long slab_floats, int ksize, int c_in, int c_out, int n_split, const float* scale, float* dw0, float* db0,
                        float* dw1, float* db1, hipStream_t s) {
    const long n_out = (long)c_out * (ksize == 3 ? 9 : ksize == 2 ? 4 : 1) * c_in + c_out;
    hipLaunchKernelGGL(wgrad_combine_kernel, dim3(cdiv(n_out, HEAD_THREADS)), dim3(HEAD_THREADS), 0, s, partial, nslab, slab_floats, ksize, c_in, c_out, n_split, scale,
                       dw0, db0, dw1, db1);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}
int wgrad_combine(const float* partial, int nslab, long slab_floats, int ksize, int c_in, int c_out, const float* scale, float* dw, float* db, hipStream_t s) {
    return wgrad_combine_split(partial, nslab, slab_floats, ksize, c_in, c_out, c_out, scale, dw, db, nullptr, nullptr, s);
}
}  // namespace detbwd
}  // namespace cosy

using namespace cosy;

extern "C" {

int cosy_head_wgrad_slab_rows(int M) { return wgrad_slab_rows(M < 0 ? 0 : M); }

size_t cosy_head_wgrad_workspace_bytes(int M, int ksize, int c_in, int c_out) {
    if (M <= 0 || c_in <= 0 || c_out <= 0 || (ksize != 1 && ksize != 2 && ksize != 3)) return 0;
    return (size_t)cdiv(M, wgrad_slab_rows(M)) * (size_t)wgrad_slab_floats(ksize, c_in, c_out) * sizeof(float);
}

int cosy_head_grad_pack(const float* g0, const float* g1, float* rows, int B, int n0, int n1, int HW, cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    COSY_REQUIRE(B >= 0 && HW >= 1, "cosy_head_grad_pack: B=%d must be >= 0 and HW=%d >= 1", B, HW);
    COSY_REQUIRE(n0 >= 0 && n1 >= 0 && n0 + n1 >= 1 && n0 + n1 <= (1 << 20), "cosy_head_grad_pack: n0=%d and n1=%d must be >= 0 and hold 1 to 2^20 columns", n0, n1);
    COSY_REQUIRE((long)B * HW <= HEAD_MAX_ROWS, "cosy_head_grad_pack: B HW = %ld rows exceed 2^30", (long)B * HW);
    if (B == 0) return COSY_OK;
    COSY_REQUIRE_PTR("cosy_head_grad_pack", rows);
    COSY_REQUIRE(((uintptr_t)rows & 15) == 0, "cosy_head_grad_pack: rows must be 16-byte aligned");
    const int GP = pad8(n0 + n1);
    const long total = (long)B * HW * GP;
    COSY_REQUIRE(cdiv(total, HEAD_THREADS) <= 0x7fffffffL && total <= (1L << 38), "cosy_head_grad_pack: %ld elements exceed 2^38", total);
    hipLaunchKernelGGL(head_grad_pack_kernel, dim3(cdiv(total, HEAD_THREADS)), dim3(HEAD_THREADS), 0, s, g0, g1, rows, n0, n1, GP, HW, total);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

int cosy_head_weight_pack(const float* w0, const float* b0, const float* w1, const float* b1, int ksize, int c_in, int n0, int n1, float* fwd,
                          float* fwd_bias, float* bwd, cosy_stream_t stream) {
    COSY_REQUIRE(ksize == 1 || ksize == 2 || ksize == 3, "cosy_head_weight_pack: ksize=%d must be 1, 3 or 2 (ConvTranspose2d(2, 2))", ksize);
    COSY_REQUIRE(c_in >= 8 && c_in % 8 == 0 && c_in <= (1 << 24), "cosy_head_weight_pack: the reduction length c_in=%d must be a positive multiple of 8", c_in);
    COSY_REQUIRE(n0 >= 1 && n1 >= 0 && (long)n0 + n1 <= (1 << 22), "cosy_head_weight_pack: n0=%d must be >= 1 and n1=%d >= 0", n0, n1);
    COSY_REQUIRE(ksize != 2 || (n1 == 0 && n0 % 8 == 0), "cosy_head_weight_pack: a deconvolution has no sibling and n0=%d a multiple of 8", n0);
    COSY_REQUIRE_PTR("cosy_head_weight_pack", w0); COSY_REQUIRE_PTR("cosy_head_weight_pack", b0);
    COSY_REQUIRE_PTR("cosy_head_weight_pack", fwd); COSY_REQUIRE_PTR("cosy_head_weight_pack", fwd_bias); COSY_REQUIRE_PTR("cosy_head_weight_pack", bwd);
    COSY_REQUIRE(n1 == 0 || (w1 != nullptr && b1 != nullptr), "cosy_head_weight_pack: null w1 or b1 with n1=%d", n1);
    return run_weight_pack("cosy_head_weight_pack", w0, b0, w1, b1, nullptr, ksize, c_in, n0, n1, fwd, fwd_bias, bwd, (hipStream_t)stream);
}

int cosy_trunk_weight_pack(const float* w, const float* scale, const float* shift, int ksize, int c_in, int c_out, float* fwd, float* fwd_bias, float* bwd,
                           cosy_stream_t stream) {
    COSY_REQUIRE(ksize == 1 || ksize == 3, "cosy_trunk_weight_pack: ksize=%d must be 1 or 3", ksize);
    COSY_REQUIRE(c_in >= 8 && c_in % 8 == 0 && c_in <= (1 << 24), "cosy_trunk_weight_pack: c_in=%d must be a positive multiple of 8", c_in);
    COSY_REQUIRE(c_out >= 8 && c_out % 8 == 0 && c_out <= (1 << 22), "cosy_trunk_weight_pack: c_out=%d must be a positive multiple of 8", c_out);
    COSY_REQUIRE_PTR("cosy_trunk_weight_pack", w); COSY_REQUIRE_PTR("cosy_trunk_weight_pack", shift);
    COSY_REQUIRE_PTR("cosy_trunk_weight_pack", fwd); COSY_REQUIRE_PTR("cosy_trunk_weight_pack", fwd_bias); COSY_REQUIRE_PTR("cosy_trunk_weight_pack", bwd);
    COSY_REQUIRE(((uintptr_t)w & 3) == 0 && ((uintptr_t)scale & 3) == 0 && ((uintptr_t)shift & 3) == 0 && ((uintptr_t)fwd & 15) == 0 && ((uintptr_t)bwd & 15) == 0 &&
                 ((uintptr_t)fwd_bias & 3) == 0, "cosy_trunk_weight_pack: w, scale, shift and fwd_bias must be 4-byte, fwd and bwd 16-byte aligned");
    return run_weight_pack("cosy_trunk_weight_pack", w, shift, nullptr, nullptr, scale, ksize, c_in, c_out, 0, fwd, fwd_bias, bwd, (hipStream_t)stream);
}

int cosy_head_dgrad(const cosy_head_layer_t* layer, const float* y, cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    COSY_REQUIRE_PTR("cosy_head_dgrad", layer);
    const cosy_head_layer_t& a = *layer;
    COSY_REQUIRE(a.dtype == COSY_F32, "cosy_head_dgrad: dtype=%d is not COSY_F32 (training is float32 only)", a.dtype);
    COSY_REQUIRE(a.ksize == 1 || a.ksize == 2 || a.ksize == 3, "cosy_head_dgrad: ksize=%d must be 1, 3 or 2 (ConvTranspose2d(2, 2))", a.ksize);
    COSY_REQUIRE(a.c_in >= 8 && a.c_in % 8 == 0, "cosy_head_dgrad: the reduction length c_in=%d must be a positive multiple of 8", a.c_in);
    COSY_REQUIRE(a.c_out >= 8 && a.c_out % 8 == 0, "cosy_head_dgrad: c_out=%d (the layer's input channels) must be a positive multiple of 8", a.c_out);
    COSY_REQUIRE(a.store == COSY_HEAD_STORE_ROWS || a.store == COSY_HEAD_STORE_NCHW, "cosy_head_dgrad: store=%d is not COSY_HEAD_STORE_ROWS or COSY_HEAD_STORE_NCHW", a.store);
    COSY_REQUIRE(a.relu == 0, "cosy_head_dgrad: relu=%d must be 0 (the mask is given by y)", a.relu);
    COSY_REQUIRE(a.store != COSY_HEAD_STORE_NCHW || (a.n_split == a.c_out && y == nullptr), "cosy_head_dgrad: an NCHW store takes n_split == c_out=%d and no y", a.c_out);
    const long rows_in = check_levels("cosy_head_dgrad", a);
    if (rows_in < 0) return COSY_EINVAL;
    long M = rows_in;
    if (a.ksize == 2) {
        COSY_REQUIRE(a.n_levels == 1 && a.H[0] % 2 == 0 && a.W[0] % 2 == 0, "cosy_head_dgrad: ksize 2 takes one level of even maps, got %d levels of %d x %d",
                     a.n_levels, a.H[0], a.W[0]);
        M = rows_in / 4;
    }
    if (M == 0) return COSY_OK;
    COSY_REQUIRE_PTR("cosy_head_dgrad", a.x); COSY_REQUIRE_PTR("cosy_head_dgrad", a.w); COSY_REQUIRE_PTR("cosy_head_dgrad", a.out);
    COSY_REQUIRE(((uintptr_t)a.x & 15) == 0 && ((uintptr_t)a.w & 15) == 0 && ((uintptr_t)a.out & 15) == 0 && ((uintptr_t)y & 15) == 0,
                 "cosy_head_dgrad: x, w, out and y must be 16-byte aligned");
    if (a.ksize == 2) return launch_deconv_dgrad(a, (int)M, y, s);
    const tadd_t<float> none{nullptr, ADD_NONE, 1, 1, 1.f, 1.f};
    return launch_dgrad_rows<float, 1>("cosy_head_dgrad", a, (int)M, tgrad_epi_t<float>{y, {none, none}, 0, 0}, s);
}

int cosy_trunk_dgrad(const cosy_head_layer_t* layer, int stride, const float* add0, int rule0, int add0_H, int add0_W, const float* add1, int rule1, int add1_H,
                     int add1_W, const float* y, cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    COSY_REQUIRE_PTR("cosy_trunk_dgrad", layer);
    const cosy_head_layer_t& a = *layer;
    COSY_REQUIRE(a.dtype == COSY_F32, "cosy_trunk_dgrad: dtype=%d is not COSY_F32 (training is float32 only)", a.dtype);
    return run_trunk_dgrad<float>("cosy_trunk_dgrad", a, stride, add0, rule0, add0_H, add0_W, add1, rule1, add1_H, add1_W, y, s);
}

int cosy_head_wgrad(const cosy_head_layer_t* layer, const float* g, float* dw0, float* db0, float* dw1, float* db1, void* workspace, size_t workspace_bytes,
                    cosy_stream_t stream) {
    COSY_REQUIRE_PTR("cosy_head_wgrad", layer);
    const cosy_head_layer_t& a = *layer;
    COSY_REQUIRE(a.dtype == COSY_F32, "cosy_head_wgrad: dtype=%d is not COSY_F32 (training is float32 only)", a.dtype);
    COSY_REQUIRE(a.ksize == 1 || a.ksize == 2 || a.ksize == 3, "cosy_head_wgrad: ksize=%d must be 1, 3 or 2 (ConvTranspose2d(2, 2))", a.ksize);
    COSY_REQUIRE(a.c_in >= 8 && a.c_in % 8 == 0, "cosy_head_wgrad: c_in=%d must be a positive multiple of 8", a.c_in);
    COSY_REQUIRE(a.c_out >= 1 && a.c_out <= (1 << 22), "cosy_head_wgrad: c_out=%d must lie in [1, 2^22]", a.c_out);
    COSY_REQUIRE(a.n_split >= 1 && a.n_split <= a.c_out, "cosy_head_wgrad: n_split=%d must lie in [1, c_out=%d]", a.n_split, a.c_out);
    COSY_REQUIRE(a.ksize != 2 || (a.n_levels == 1 && a.n_split == a.c_out && a.c_out % 8 == 0),
                 "cosy_head_wgrad: ksize 2 takes one level, no sibling and c_out=%d a multiple of 8", a.c_out);
    const long M = check_levels("cosy_head_wgrad", a);
    if (M < 0) return COSY_EINVAL;
    COSY_REQUIRE(a.ksize != 2 || 4 * M <= HEAD_MAX_ROWS, "cosy_head_wgrad: 4 x %ld gradient rows exceed 2^30", M);
    COSY_REQUIRE_PTR("cosy_head_wgrad", dw0); COSY_REQUIRE_PTR("cosy_head_wgrad", db0);
    COSY_REQUIRE(a.n_split == a.c_out || (dw1 != nullptr && db1 != nullptr), "cosy_head_wgrad: null dw1 or db1 with n_split=%d < c_out=%d", a.n_split, a.c_out);
    const int T = a.ksize == 3 ? 9 : a.ksize == 2 ? 4 : 1;
    COSY_REQUIRE((long)a.c_out * T * a.c_in + a.c_out <= (1L << 36), "cosy_head_wgrad: c_out=%d x c_in=%d weights exceed 2^36", a.c_out, a.c_in);
    return run_wgrad("cosy_head_wgrad", a, 1, M, g, nullptr, a.n_split, dw0, db0, dw1, db1, workspace, workspace_bytes, (hipStream_t)stream);
}

int cosy_trunk_wgrad(const cosy_head_layer_t* layer, int stride, const float* g, const float* scale, float* dw, float* db, void* workspace, size_t workspace_bytes,
                     cosy_stream_t stream) {
    COSY_REQUIRE_PTR("cosy_trunk_wgrad", layer);
    const cosy_head_layer_t& a = *layer;
    COSY_REQUIRE(a.dtype == COSY_F32, "cosy_trunk_wgrad: dtype=%d is not COSY_F32 (training is float32 only)", a.dtype);
    COSY_REQUIRE(a.ksize == 1 || a.ksize == 3, "cosy_trunk_wgrad: ksize=%d must be 1 or 3", a.ksize);
    COSY_REQUIRE(stride == 1 || stride == 2, "cosy_trunk_wgrad: stride=%d must be 1 or 2", stride);
    COSY_REQUIRE(a.c_in >= 8 && a.c_in % 8 == 0, "cosy_trunk_wgrad: c_in=%d must be a positive multiple of 8", a.c_in);
    COSY_REQUIRE(a.c_out >= 8 && a.c_out % 8 == 0 && a.c_out <= (1 << 22), "cosy_trunk_wgrad: c_out=%d must be a positive multiple of 8", a.c_out);
    const long M_in = check_levels("cosy_trunk_wgrad", a);
    if (M_in < 0) return COSY_EINVAL;
    COSY_REQUIRE(stride == 1 || a.n_levels == 1, "cosy_trunk_wgrad: stride=2 takes one level, got n_levels=%d", a.n_levels);
    const int Ho = (a.H[0] - 1) / stride + 1, Wo = (a.W[0] - 1) / stride + 1;
    const long T = stride == 1 ? M_in : M_in / ((long)a.H[0] * a.W[0]) * Ho * Wo;       // the OUTPUT cells: the k dimension
    COSY_REQUIRE_PTR("cosy_trunk_wgrad", dw);
    COSY_REQUIRE(((uintptr_t)dw & 3) == 0 && ((uintptr_t)db & 3) == 0 && ((uintptr_t)scale & 3) == 0 && ((uintptr_t)g & 3) == 0 && ((uintptr_t)workspace & 3) == 0,
                 "cosy_trunk_wgrad: g, scale, dw, db and workspace must be 4-byte aligned");
    COSY_REQUIRE((long)a.c_out * (a.ksize == 3 ? 9 : 1) * a.c_in <= (1L << 36), "cosy_trunk_wgrad: c_out=%d x c_in=%d weights exceed 2^36", a.c_out, a.c_in);
    return run_wgrad("cosy_trunk_wgrad", a, stride, T, g, scale, a.c_out, dw, db, nullptr, nullptr, workspace, workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
