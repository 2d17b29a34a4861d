// The backward of the detector on the matrix pipe: the heads and the trunk (section 29) run ONE set of gradient kernels,
// and every entry point of the backward is here, the float32 rows' and the bfloat16 rows' (`16`, sections 30 and 32) side by side: an entry checks
// its layer pointer and dtype and calls the body that both row types share (run_*<T> below and in detbwd_device.h).  The parameters are float32
// whatever the rows are.  A layer is v = conv_stride(x, W) [scale + shift] [+ r], y = act(v) (kernels_dethead.hip, kernels_dettrunk.hip); g is
// the gradient at v, rows on the layer's OUTPUT grid (heads: c_out rounded up to 8, the pad +0.0).  What follows describes the float32 rows.
//   * data gradient   dX[cell][c] = sum over (tap, o) of w[o][tap][c] g[cell - tap][o]: detbwd_device.h's dgrad_rows_kernel<float>, the forward GEMM's chain (dethead_device.h:
//     accumulator +0.0, blocks of 16 o ascending, the taps of the flipped packing ascending inside a block, every term one fmaf) over the rows g
//     with the weight transposed and its taps flipped.  At stride 2 a launch owns ONE parity class of (iy, ix) and runs only that class's live
//     taps (1, 2, 2 or 4 of 9).  Its store adds up to two operands (SAME, EVEN, NEAREST_T: the trunk's shortcuts and the FPN), applies the ReLU
//     mask of the layer below and writes rows or NCHW, so the launch writes that layer's pre-activation gradient.  ConvTranspose2d(2, 2) alone
//     stays on conv_gemm_kernel (DeconvGradPolicyOf<T>): its four stride-2 taps over the rows of the (2H, 2W) map.
//   * weight gradient dW[o][tap][c] = [scale[o]] sum over OUTPUT cells of g[(y, x)][o] x[(stride y + dy, stride x + dx)][c], bias gradient
//     db[o] = sum over cells of g[cell][o]: wgrad_kernel, v_mfma_f32_16x16x4_f32 with the CELLS as the k dimension, streamed once.  The cells are
//     cut into slabs (cosy_head_wgrad_slab_rows); a wave writes its slab's partial tile, wgrad_combine_kernel adds the slabs in ascending order,
//     multiplies by scale[o] once and writes torchvision's layout.  No atomics: two calls give equal bits.  bfloat16 rows: the first pass is
//     kernels_detbwd16.hip's wgrad16_kernel (launch_wgrad); slabs, workspace and second pass are the same.
//   * head_grad_pack_kernel / grad_pack16_kernel make the rows g out of the losses' NCHW gradients; weight_pack_kernel<T> makes both
//     fragment-order weights (forward, and transposed + flipped [x scale[o], rounded once] for the data gradient) out of a parameter in
//     torchvision's layout, on the device.
// No atomics, no LDS: equal inputs give equal bits.
#include "detbwd_device.h"

namespace cosy {
namespace {

using namespace headgemm;
using namespace detbwd;                      // the data gradient: kernel, store rules and entry checks, one template over the type of the rows

constexpr int WG_SLAB_MIN = 256;             // cells of a slab: at least this many, and at most WG_MAX_SLABS slabs
constexpr int WG_MAX_SLABS = 16;

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

// the same on bfloat16 rows.  One thread: eight columns of one cell; neighbouring threads take neighbouring cells of the same columns
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

// the weight packs of the heads and the trunk: one thread per element of [fwd | bwd | fwd_bias]; the rules are detbwd_device.h's weight_pack_element
// (float32 packings: 16 of the reduction per block, four elements per lane; bfloat16: 32 and eight, one float32 product with scale, then ONE rounding)
template <typename T>
__global__ __launch_bounds__(HEAD_THREADS) void weight_pack_kernel(const float* __restrict__ w0, const float* __restrict__ b0, const float* __restrict__ w1,
                                                                   const float* __restrict__ b1, const float* __restrict__ scale, int ksize, int C, int n0, int n1,
                                                                   T* __restrict__ fwd, float* __restrict__ fwd_bias, T* __restrict__ bwd, long n_fwd, long n_bwd,
                                                                   int n_bias) {
    weight_pack_element<T>((long)blockIdx.x * HEAD_THREADS + threadIdx.x, w0, b0, w1, b1, scale, ksize, C, n0, n1, fwd, fwd_bias, bwd, n_fwd, n_bwd, n_bias);
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

// One weight gradient on rows of T, planned and launched, after the caller's checks of the layer's shape: M OUTPUT cells (the k dimension) of a
// layer a.c_in -> a.c_out at `stride`; outputs [0, n_split) go to dw0 / db0 (db0 null: no bias gradient), the rest to dw1 / db1.  The rows g hold
// pad8(c_out) columns (the heads' pad columns +0.0; the trunk and a deconvolution have c_out a multiple of 8).  M == 0: zeros of the right shape.
template <typename T>
int run_wgrad(const char* fn, const cosy_head_layer_t& a, int stride, long M, const T* g, const float* scale, int n_split, float* dw0, float* db0, float* dw1,
              float* db1, void* workspace, size_t workspace_bytes, hipStream_t s) {
    const int taps = a.ksize == 3 ? 9 : a.ksize == 2 ? 4 : 1;
    COSY_REQUIRE(a.c_in >= 8 && a.c_in % 8 == 0, "%s: c_in=%d must be a positive multiple of 8", fn, a.c_in);
    COSY_REQUIRE((long)a.c_out * taps * a.c_in + a.c_out <= (1L << 36), "%s: c_out=%d x c_in=%d weights exceed 2^36", fn, a.c_out, a.c_in);
    COSY_REQUIRE(dw0 != nullptr, "%s: null dw0", fn);
    COSY_REQUIRE(n_split == a.c_out || (dw1 != nullptr && db1 != nullptr), "%s: null dw1 or db1 with n_split=%d < c_out=%d", fn, n_split, a.c_out);
    COSY_REQUIRE(aligned(dw0, 4) && aligned(db0, 4) && aligned(dw1, 4) && aligned(db1, 4) && aligned(scale, 4) && aligned(workspace, 4),
                 "%s: dw0, db0, dw1, db1, scale and workspace must be 4-byte aligned", fn);
    if (M == 0) {
        const long nw0 = (long)n_split * taps * a.c_in, nw1 = (long)(a.c_out - n_split) * taps * a.c_in;
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
    constexpr int row_align = sizeof(T) == 4 ? 4 : 16;         // float32 rows are read by the element, 16-bit rows eight at a time
    COSY_REQUIRE(aligned(a.x, row_align) && aligned(g, row_align), "%s: the rows x and g must be %d-byte aligned", fn, row_align);
    wgrad_plan_t p;
    p.GP = pad8(a.c_out); p.M = (int)M; p.want_db = db0 != nullptr; p.partial = (float*)workspace;
    p.slab = wgrad_slab_rows(p.M); p.nslab = cdiv(M, p.slab);
    p.slab_floats = wgrad_slab_floats(a.ksize, a.c_in, a.c_out);
    const size_t need = (size_t)p.nslab * (size_t)p.slab_floats * sizeof(float);
    COSY_REQUIRE(workspace_bytes >= need, "%s: workspace_bytes=%zu is less than the %zu bytes that %ld cells of c_in=%d, c_out=%d need "
                 "(cosy_head_wgrad_workspace_bytes)", fn, workspace_bytes, need, M, a.c_in, a.c_out);
    p.c_groups = cdiv(a.c_in, wgrad_group_channels<T>(a.ksize));
    const long n_waves = (long)cdiv(a.c_out, 16) * p.c_groups;
    COSY_REQUIRE(n_waves <= 0x7fffffffL, "%s: c_out=%d x c_in=%d need more than 2^31 - 1 waves", fn, a.c_out, a.c_in);
    p.n_waves = (int)n_waves;
    launch_wgrad(a, stride, g, p, s);
    COSY_CHECK_HIP(hipGetLastError());
    const long n_out = (long)a.c_out * taps * a.c_in + a.c_out;
    hipLaunchKernelGGL(wgrad_combine_kernel, dim3(cdiv(n_out, HEAD_THREADS)), dim3(HEAD_THREADS), 0, s, p.partial, p.nslab, p.slab_floats, a.ksize, a.c_in, a.c_out, n_split,
                       scale, dw0, db0, dw1, db1);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

// cosy_head_wgrad's contract (cosyhip.h) on rows of T, after the caller's check of the layer pointer and of dtype
template <typename T>
int run_head_wgrad(const char* fn, const cosy_head_layer_t& a, const T* g, float* dw0, float* db0, float* dw1, float* db1, void* workspace, size_t workspace_bytes,
                   hipStream_t s) {
    COSY_REQUIRE(a.ksize == 1 || a.ksize == 2 || a.ksize == 3, "%s: ksize=%d must be 1, 3 or 2 (ConvTranspose2d(2, 2))", fn, a.ksize);
    COSY_REQUIRE(a.c_out >= 1 && a.c_out <= (1 << 22), "%s: c_out=%d must lie in [1, 2^22]", fn, a.c_out);
    COSY_REQUIRE(a.n_split >= 1 && a.n_split <= a.c_out, "%s: n_split=%d must lie in [1, c_out=%d]", fn, a.n_split, a.c_out);
    COSY_REQUIRE(a.ksize != 2 || (a.n_levels == 1 && a.n_split == a.c_out && a.c_out % 8 == 0), "%s: ksize 2 takes one level, no sibling and c_out=%d a multiple of 8", fn,
                 a.c_out);
    const long M = check_levels(fn, a);
    if (M < 0) return COSY_EINVAL;
    COSY_REQUIRE(a.ksize != 2 || 4 * M <= HEAD_MAX_ROWS, "%s: 4 x %ld gradient rows exceed 2^30", fn, M);
    COSY_REQUIRE(db0 != nullptr, "%s: null db0", fn);
    return run_wgrad<T>(fn, a, 1, M, g, nullptr, a.n_split, dw0, db0, dw1, db1, workspace, workspace_bytes, s);
}

// cosy_trunk_wgrad's contract (cosyhip.h) on rows of T, after the caller's check of the layer pointer and of dtype
template <typename T>
int run_trunk_wgrad(const char* fn, const cosy_head_layer_t& a, int stride, const T* g, const float* scale, float* dw, float* db, void* workspace, size_t workspace_bytes,
                    hipStream_t s) {
    COSY_REQUIRE(a.ksize == 1 || a.ksize == 3, "%s: ksize=%d must be 1 or 3", fn, a.ksize);
    COSY_REQUIRE(stride == 1 || stride == 2, "%s: stride=%d must be 1 or 2", fn, stride);
    COSY_REQUIRE(a.c_out >= 8 && a.c_out % 8 == 0 && a.c_out <= (1 << 22), "%s: c_out=%d must be a positive multiple of 8", fn, a.c_out);
    const long M_in = check_levels(fn, a);
    if (M_in < 0) return COSY_EINVAL;
    COSY_REQUIRE(stride == 1 || a.n_levels == 1, "%s: stride=2 takes one level, got n_levels=%d", fn, a.n_levels);
    const int Ho = (a.H[0] - 1) / stride + 1, Wo = (a.W[0] - 1) / stride + 1;
    const long M = stride == 1 ? M_in : M_in / ((long)a.H[0] * a.W[0]) * Ho * Wo;       // the OUTPUT cells: the k dimension
    return run_wgrad<T>(fn, a, stride, M, g, scale, a.c_out, dw, db, nullptr, nullptr, workspace, workspace_bytes, s);
}

// one weight pack with packings of T, checked and launched: n0 (+ n1 sibling) outputs of c_in channels
template <typename T>
int run_weight_pack(const char* fn, const float* w0, const float* b0, const float* w1, const float* b1, const float* scale, int ksize, int c_in, int n0, int n1,
                    void* fwd, float* fwd_bias, void* bwd, hipStream_t s) {
    pack_sizes_t z;
    if (const int rc = check_weight_pack(fn, w0, b0, w1, b1, scale, fwd, fwd_bias, bwd, ksize, c_in, n0, n1, pack_frag<T>::KB, &z)) return rc;
    hipLaunchKernelGGL(weight_pack_kernel<T>, dim3(cdiv(z.n_fwd + z.n_bwd + z.n_bias, HEAD_THREADS)), dim3(HEAD_THREADS), 0, s, w0, b0, w1, b1, scale, ksize, c_in, n0, n1,
                       (T*)fwd, fwd_bias, (T*)bwd, z.n_fwd, z.n_bwd, (int)z.n_bias);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

// a trunk layer is the pack's case n1 = 0, b0 = shift, and always a 1x1 or 3x3 convolution of a multiple of 8 outputs, with a scale or without
template <typename T>
int run_trunk_weight_pack(const char* fn, const float* w, const float* scale, const float* shift, int ksize, int c_in, int c_out, void* fwd, float* fwd_bias, void* bwd,
                          hipStream_t s) {
    COSY_REQUIRE(ksize == 1 || ksize == 3, "%s: ksize=%d must be 1 or 3", fn, ksize);
    COSY_REQUIRE(c_out >= 8 && c_out % 8 == 0, "%s: c_out=%d must be a positive multiple of 8", fn, c_out);
    return run_weight_pack<T>(fn, w, shift, nullptr, nullptr, scale, ksize, c_in, c_out, 0, fwd, fwd_bias, bwd, s);
}

// one gradient pack to rows of T: one thread per element (float32) or per eight columns of a cell (bfloat16), two kernels
template <typename T> int run_grad_pack(const char* fn, const float* g0, const float* g1, void* rows, int B, int n0, int n1, int HW, hipStream_t s) {
    const long total = check_grad_pack(fn, g0, g1, rows, B, n0, n1, HW);
    if (total <= 0) return total < 0 ? COSY_EINVAL : COSY_OK;
    const int GP = pad8(n0 + n1);
    if constexpr (sizeof(T) == 4)
        hipLaunchKernelGGL(head_grad_pack_kernel, dim3(cdiv(total, HEAD_THREADS)), dim3(HEAD_THREADS), 0, s, g0, g1, (float*)rows, n0, n1, GP, HW, total);
    else
        hipLaunchKernelGGL(grad_pack16_kernel, dim3(cdiv(total / 8, HEAD_THREADS)), dim3(HEAD_THREADS), 0, s, g0, g1, (bf16_t*)rows, n0, n1, GP, HW, total / 8);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

// the dtype refusals differ on purpose: the float32 entries say where 16-bit rows go, the 16-bit entries why float16 has none
#define COSY_REQUIRE_F32(fn, dtype) COSY_REQUIRE((dtype) == COSY_F32, fn ": dtype=%d is not COSY_F32 (training is float32 only)", (dtype))
#define COSY_REQUIRE_BF16(fn, dtype, other) \
    COSY_REQUIRE((dtype) == COSY_BF16, fn ": dtype=%d is not COSY_BF16 (float32 rows: " other "; float16 training needs a loss scaler, which is not built)", (dtype))

}  // namespace

// the float32 rows' first pass; the bfloat16 rows' is kernels_detbwd16.hip's
void detbwd::launch_wgrad(const cosy_head_layer_t& a, int stride, const float* g, const wgrad_plan_t& p, hipStream_t s) {
    const dim3 grid((unsigned)cdiv(p.n_waves, HEAD_THREADS / 64), (unsigned)p.nslab), block(HEAD_THREADS);
#define COSY_WGRAD_LAUNCH(MODE, STRIDE) \
    hipLaunchKernelGGL((wgrad_kernel<MODE, STRIDE>), grid, block, 0, s, a, g, p.GP, p.M, p.slab, p.n_waves, p.c_groups, p.want_db, p.partial, p.slab_floats)
    if (a.ksize == 2) COSY_WGRAD_LAUNCH(2, 1);
    else if (a.ksize == 1 && stride == 1) COSY_WGRAD_LAUNCH(0, 1);
    else if (a.ksize == 1) COSY_WGRAD_LAUNCH(0, 2);
    else if (stride == 1) COSY_WGRAD_LAUNCH(1, 1);
    else COSY_WGRAD_LAUNCH(1, 2);
#undef COSY_WGRAD_LAUNCH
}

}  // namespace cosy

using namespace cosy;

// Every entry below checks its layer pointer, refuses the wrong dtype in its own words and calls the body that both row types share.
extern "C" {

int cosy_head_wgrad_slab_rows(int M) { return wgrad_slab_rows(M < 0 ? 0 : M); }

size_t cosy_head_wgrad_workspace_bytes(int M, int ksize, int c_in, int c_out) {
    if (M <= 0 || c_in <= 0 || c_out <= 0 || (ksize != 1 && ksize != 2 && ksize != 3)) return 0;
    return (size_t)cdiv(M, wgrad_slab_rows(M)) * (size_t)wgrad_slab_floats(ksize, c_in, c_out) * sizeof(float);
}

int cosy_head_grad_pack(const float* g0, const float* g1, float* rows, int B, int n0, int n1, int HW, cosy_stream_t stream) {
    return run_grad_pack<float>("cosy_head_grad_pack", g0, g1, rows, B, n0, n1, HW, (hipStream_t)stream);
}
int cosy_head_grad_pack16(const float* g0, const float* g1, void* rows, int B, int n0, int n1, int HW, cosy_stream_t stream) {
    return run_grad_pack<bf16_t>("cosy_head_grad_pack16", g0, g1, rows, B, n0, n1, HW, (hipStream_t)stream);
}
int cosy_trunk_grad_pack16(const float* g, void* rows, int B, int C, int HW, cosy_stream_t stream) {
    COSY_REQUIRE(C >= 8 && C % 8 == 0, "cosy_trunk_grad_pack16: C=%d must be a positive multiple of 8", C);
    return run_grad_pack<bf16_t>("cosy_trunk_grad_pack16", g, nullptr, rows, B, C, 0, HW, (hipStream_t)stream);
}

int cosy_head_weight_pack(const float* w0, const float* b0, const float* w1, const float* b1, int ksize, int c_in, int n0, int n1, float* fwd, float* fwd_bias,
                          float* bwd, cosy_stream_t stream) {
    return run_weight_pack<float>("cosy_head_weight_pack", w0, b0, w1, b1, nullptr, ksize, c_in, n0, n1, fwd, fwd_bias, bwd, (hipStream_t)stream);
}
int cosy_head_weight_pack16(const float* w0, const float* b0, const float* w1, const float* b1, int ksize, int c_in, int n0, int n1, void* fwd, float* fwd_bias,
                            void* bwd, cosy_stream_t stream) {
    return run_weight_pack<bf16_t>("cosy_head_weight_pack16", w0, b0, w1, b1, nullptr, ksize, c_in, n0, n1, fwd, fwd_bias, bwd, (hipStream_t)stream);
}
int cosy_trunk_weight_pack(const float* w, const float* scale, const float* shift, int ksize, int c_in, int c_out, float* fwd, float* fwd_bias, float* bwd,
                           cosy_stream_t stream) {
    return run_trunk_weight_pack<float>("cosy_trunk_weight_pack", w, scale, shift, ksize, c_in, c_out, fwd, fwd_bias, bwd, (hipStream_t)stream);
}
int cosy_trunk_weight_pack16(const float* w, const float* scale, const float* shift, int ksize, int c_in, int c_out, void* fwd, float* fwd_bias, void* bwd,
                             cosy_stream_t stream) {
    return run_trunk_weight_pack<bf16_t>("cosy_trunk_weight_pack16", w, scale, shift, ksize, c_in, c_out, fwd, fwd_bias, bwd, (hipStream_t)stream);
}

int cosy_head_dgrad(const cosy_head_layer_t* layer, const float* y, cosy_stream_t stream) {
    COSY_REQUIRE_PTR("cosy_head_dgrad", layer);
    COSY_REQUIRE_F32("cosy_head_dgrad", layer->dtype);
    return run_head_dgrad<float>("cosy_head_dgrad", *layer, y, (hipStream_t)stream);
}
int cosy_head_dgrad16(const cosy_head_layer_t* layer, const void* y, cosy_stream_t stream) {
    COSY_REQUIRE_PTR("cosy_head_dgrad16", layer);
    COSY_REQUIRE_BF16("cosy_head_dgrad16", layer->dtype, "cosy_head_dgrad");
    return run_head_dgrad<bf16_t>("cosy_head_dgrad16", *layer, (const bf16_t*)y, (hipStream_t)stream);
}

int cosy_trunk_dgrad(const cosy_head_layer_t* layer, int stride, const float* add0, int rule0, int add0_H, int add0_W, const float* add1, int rule1, int add1_H,
                     int add1_W, const float* y, cosy_stream_t stream) {
    COSY_REQUIRE_PTR("cosy_trunk_dgrad", layer);
    COSY_REQUIRE_F32("cosy_trunk_dgrad", layer->dtype);
    return run_trunk_dgrad<float>("cosy_trunk_dgrad", *layer, stride, add0, rule0, add0_H, add0_W, add1, rule1, add1_H, add1_W, y, (hipStream_t)stream);
}
int cosy_trunk_dgrad16(const cosy_head_layer_t* layer, int stride, const void* add0, int rule0, int add0_H, int add0_W, const void* add1, int rule1, int add1_H,
                       int add1_W, const void* y, cosy_stream_t stream) {
    COSY_REQUIRE_PTR("cosy_trunk_dgrad16", layer);
    COSY_REQUIRE_BF16("cosy_trunk_dgrad16", layer->dtype, "cosy_trunk_dgrad");
    return run_trunk_dgrad<bf16_t>("cosy_trunk_dgrad16", *layer, stride, (const bf16_t*)add0, rule0, add0_H, add0_W, (const bf16_t*)add1, rule1, add1_H, add1_W,
                                   (const bf16_t*)y, (hipStream_t)stream);
}

int cosy_head_wgrad(const cosy_head_layer_t* layer, const float* g, float* dw0, float* db0, float* dw1, float* db1, void* workspace, size_t workspace_bytes,
                    cosy_stream_t stream) {
    COSY_REQUIRE_PTR("cosy_head_wgrad", layer);
    COSY_REQUIRE_F32("cosy_head_wgrad", layer->dtype);
    return run_head_wgrad<float>("cosy_head_wgrad", *layer, g, dw0, db0, dw1, db1, workspace, workspace_bytes, (hipStream_t)stream);
}
int cosy_head_wgrad16(const cosy_head_layer_t* layer, const void* g, float* dw0, float* db0, float* dw1, float* db1, void* workspace, size_t workspace_bytes,
                      cosy_stream_t stream) {
    COSY_REQUIRE_PTR("cosy_head_wgrad16", layer);
    COSY_REQUIRE_BF16("cosy_head_wgrad16", layer->dtype, "cosy_head_wgrad");
    return run_head_wgrad<bf16_t>("cosy_head_wgrad16", *layer, (const bf16_t*)g, dw0, db0, dw1, db1, workspace, workspace_bytes, (hipStream_t)stream);
}

int cosy_trunk_wgrad(const cosy_head_layer_t* layer, int stride, const float* g, const float* scale, float* dw, float* db, void* workspace, size_t workspace_bytes,
                     cosy_stream_t stream) {
    COSY_REQUIRE_PTR("cosy_trunk_wgrad", layer);
    COSY_REQUIRE_F32("cosy_trunk_wgrad", layer->dtype);
    return run_trunk_wgrad<float>("cosy_trunk_wgrad", *layer, stride, g, scale, dw, db, workspace, workspace_bytes, (hipStream_t)stream);
}
int cosy_trunk_wgrad16(const cosy_head_layer_t* layer, int stride, const void* g, const float* scale, float* dw, float* db, void* workspace, size_t workspace_bytes,
                       cosy_stream_t stream) {
    COSY_REQUIRE_PTR("cosy_trunk_wgrad16", layer);
    COSY_REQUIRE_BF16("cosy_trunk_wgrad16", layer->dtype, "cosy_trunk_wgrad");
    return run_trunk_wgrad<bf16_t>("cosy_trunk_wgrad16", *layer, stride, (const bf16_t*)g, scale, dw, db, workspace, workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
