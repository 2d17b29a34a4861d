// The backward of the detector's heads on the matrix pipe, float32 only.  For one layer y = act(W x + b) of
// kernels_dethead.hip and the gradient g at its pre-activation output, as rows (M, c_out rounded up to 8, the pad +0.0):
//   * data gradient   dX[cell][c] = sum over (tap, o) of w[o][tap][c] g[cell - tap][o]: the FORWARD GEMM (dethead_device.h) run on the rows g
//     with the weight transposed and its taps flipped (GradPolicy); its row store applies the ReLU mask of the layer below, so the launch writes
//     that layer's pre-activation gradient; ConvTranspose2d(2, 2): the four stride-2 taps over the rows of the (2H, 2W) map;
//   * weight gradient dW[o][tap][c] = sum over cells of g[cell][o] x[cell + tap][c], bias gradient db[o] = sum over cells of g[cell][o]:
//     head_wgrad_kernel, v_mfma_f32_16x16x4_f32 with the CELLS as the k dimension, streamed once.  The cells are cut into slabs
//     (cosy_head_wgrad_slab_rows); a wave writes its slab's partial tile, head_wgrad_combine_kernel adds the slabs in ascending order and
//     writes torchvision's layout.  No atomics: two calls give equal bits.
// head_grad_pack_kernel makes the rows g out of the losses' NCHW gradients, head_weight_pack_kernel makes both fragment-order weights
// (forward, and transposed + flipped for the data gradient) out of a parameter in torchvision's layout, on the device.
#include "dethead_device.h"

namespace cosy {
namespace {

using namespace headgemm;

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

// the element (o, tap, c) of a layer's weight in torchvision's layout; o runs over the first tensor's outputs, then the second's.
// ksize 1 / 3: (O, C, k, k) or (O, C); ksize 2: ConvTranspose2d's (C, O, 2, 2)
__device__ __forceinline__ float weight_at(const float* __restrict__ w0, const float* __restrict__ w1, int ksize, int C, int n0, int n1, int o, int tap, int c) {
    if (ksize == 2) return w0[((long)c * n0 + o) * 4 + tap];
    const int T = ksize == 3 ? 9 : 1;
    return o < n0 ? w0[((long)o * C + c) * T + tap] : w1[((long)(o - n0) * C + c) * T + tap];
}

// fragment order of cosy_head_conv, float32: element [nt][tap][kb][lane][e] holds W[16 nt + (lane & 15)][tap][16 kb + 4 (lane >> 4) + e].
// forward: W = the layer's (rows o; ksize 2: rows (o, dy, dx), one tap); backward: rows c, reduction o, taps flipped (ksize 3) or (dy, dx) (ksize 2).
__global__ __launch_bounds__(HEAD_THREADS) void head_weight_pack_kernel(const float* __restrict__ w0, const float* __restrict__ b0, const float* __restrict__ w1,
                                                                        const float* __restrict__ b1, int ksize, int C, int n0, int n1, float* __restrict__ fwd,
                                                                        float* __restrict__ fwd_bias, float* __restrict__ bwd, long n_fwd, long n_bwd, int n_bias) {
    const long i = (long)blockIdx.x * HEAD_THREADS + threadIdx.x;
    const int O = n0 + n1;
    if (i < n_fwd + n_bwd) {
        const bool back = i >= n_fwd;
        const long k = back ? i - n_fwd : i;
        const int taps = back ? (ksize == 3 ? 9 : ksize == 2 ? 4 : 1) : (ksize == 3 ? 9 : 1);
        const int N = back ? C : (ksize == 2 ? 4 * O : O), K = back ? O : C;           // rows and reduction length of this packing
        const int KBn = (K + 15) / 16;
        const int e = (int)(k & 3), lane = (int)((k >> 2) & 63);
        const long s = k >> 8;
        const int kb = (int)(s % KBn), tap = (int)((s / KBn) % taps), nt = (int)(s / ((long)KBn * taps));
        const int n = 16 * nt + (lane & 15), r = 16 * kb + 4 * (lane >> 4) + e;
        float v = 0.f;
        if (n < N && r < K) {
            if (!back) v = ksize == 2 ? weight_at(w0, w1, 2, C, n0, n1, n >> 2, n & 3, r) : weight_at(w0, w1, ksize, C, n0, n1, n, tap, r);
            else v = weight_at(w0, w1, ksize, C, n0, n1, r, ksize == 3 ? 8 - tap : tap, n);
        }
        (back ? bwd : fwd)[k] = v;
    } else if (i < n_fwd + n_bwd + n_bias) {
        const int n = (int)(i - n_fwd - n_bwd);
        const int o = ksize == 2 ? n >> 2 : n;
        float v = 0.f;
        if (o < O) v = o < n0 ? b0[o] : b1[o - n0];
        fwd_bias[n] = v;
    }
}

// MODE 0: one tap (1x1 conv, linear); 1: 3x3, pad 1; 2: ConvTranspose2d(2, 2).  A wave owns 16 outputs o x 16 CT channels c x all taps of one
// slab of cells.  The MFMA's A operand is g^T (row o = lane & 15, k = the cell lane >> 4), its B operand x (k = the cell, column c = lane & 15),
// four cells per instruction; the result has o = 4 (lane >> 4) + reg, c = lane & 15.  The bias gradient is the same product against a column of
// ones, taken by the waves of channel group 0.  A cell past the slab, a tap outside the map and a column past the row feed +0.0; no address is formed.
template <int MODE>
__global__ __launch_bounds__(HEAD_THREADS) void head_wgrad_kernel(const cosy_head_layer_t a, const float* __restrict__ g, const int GP, const int M, const int slab,
                                                                  const int n_waves, const int c_groups, float* __restrict__ partial, const long slab_floats) {
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

    f32x4 acc[TAPS][CT], accb = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < TAPS; ++t)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) acc[t][ct] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (long k0 = k_begin; k0 < k_end; k0 += 4) {
        const long cell = k0 + kq;
        const bool in = cell < k_end;
        if constexpr (MODE == 0) {
            const float av = in && o_in ? g[cell * GP + o_a] : 0.f;
            float bv[CT];
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                const int c = (cg * CT + ct) * 16 + j;
                bv[ct] = in && c < C ? x[cell * C + c] : 0.f;
            }
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) acc[0][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[ct], acc[0][ct], 0, 0, 0);
            if (cg == 0) accb = __builtin_amdgcn_mfma_f32_16x16x4f32(av, 1.f, accb, 0, 0, 0);
        } else if constexpr (MODE == 1) {
            const float av = in && o_in ? g[cell * GP + o_a] : 0.f;
            const int c = cg * 16 + j;
            int H = 0, W = 0, py = 0, px = 0;                  // H = 0: no tap is inside
            if (in && c < C) {
                int l = 0;
                while (l + 1 < a.n_levels && cell >= a.row_start[l + 1]) ++l;
                H = a.H[l]; W = a.W[l];
                const int pix = (int)((cell - a.row_start[l]) % ((long)H * W));
                py = pix / W; px = pix - py * W;
            }
            float bv[TAPS];
#pragma unroll
            for (int t = 0; t < TAPS; ++t) {
                const int dy = t / 3 - 1, dx = t - (t / 3) * 3 - 1;
                const bool tin = (unsigned)(py + dy) < (unsigned)H && (unsigned)(px + dx) < (unsigned)W;
                bv[t] = tin ? x[(cell + dy * W + dx) * C + c] : 0.f;
            }
#pragma unroll
            for (int t = 0; t < TAPS; ++t) acc[t][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[t], acc[t][0], 0, 0, 0);
            if (cg == 0) accb = __builtin_amdgcn_mfma_f32_16x16x4f32(av, 1.f, accb, 0, 0, 0);
        } else {
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
            if (cg == 0)
#pragma unroll
                for (int t = 0; t < TAPS; ++t) accb = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t], 1.f, accb, 0, 0, 0);
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
    if (cg == 0 && j == 0)
#pragma unroll
        for (int q = 0; q < 4; ++q) out[O16 * TAPS * C + ot * 16 + 4 * kq + q] = accb[q];
}

// slab 0, then + slab 1, + slab 2, ...: one thread per element of the results, which it writes in torchvision's layout:
// ksize 1 / 3: (O, C, k, k), outputs [0, n_split) to dw0 / db0 and the rest to dw1 / db1; ksize 2: (C, O, 2, 2)
__global__ __launch_bounds__(HEAD_THREADS) void head_wgrad_combine_kernel(const float* __restrict__ partial, int nslab, long slab_floats, int ksize, int C, int O,
                                                                          int n_split, float* __restrict__ dw0, float* __restrict__ db0,
                                                                          float* __restrict__ dw1, float* __restrict__ db1) {
    const int T = ksize == 3 ? 9 : ksize == 2 ? 4 : 1;
    const long n_w = (long)O * T * C, O16 = (long)((O + 15) / 16) * 16;
    const long i = (long)blockIdx.x * HEAD_THREADS + threadIdx.x;
    if (i >= n_w + O) return;
    const long src = i < n_w ? i : O16 * T * C + (i - n_w);
    float acc = partial[src];
    for (int s = 1; s < nslab; ++s) acc = acc + partial[(long)s * slab_floats + src];
    if (i >= n_w) {
        const int o = (int)(i - n_w);
        if (o < n_split) db0[o] = acc; else db1[o - n_split] = acc;
        return;
    }
    const int o = (int)(i / ((long)T * C)), t = (int)((i / C) % T), c = (int)(i % C);
    if (ksize == 2) dw0[((long)c * O + o) * 4 + t] = acc;
    else if (o < n_split) dw0[((long)o * C + c) * T + t] = acc;
    else dw1[((long)(o - n_split) * C + c) * T + t] = acc;
}

int launch_head_dgrad(const cosy_head_layer_t& a, int M, const float* y, hipStream_t s) {
    const conv_grid_t c = conv_grid<float>(a, M);
    COSY_REQUIRE(c.blocks <= 0x7fffffffL, "cosy_head_dgrad: %d rows x c_out=%d need more than 2^31 - 1 workgroups", M, a.c_out);
    const dim3 grid((unsigned)c.blocks), block(HEAD_THREADS);
    const int KBn = c.KBn, n_tiles = c.n_tiles, ng = c.n_groups;
    const grad_epi_t e{y};
#define COSY_DGRAD_LAUNCH(P)                                                                                                                         \
    do {                                                                                                                                             \
        if (c.big_m && c.big_n) hipLaunchKernelGGL((conv_gemm_kernel<float, TILE_MT_BIG, TILE_NT_BIG, P>), grid, block, 0, s, a, M, KBn, n_tiles, ng, e); \
        else if (c.big_m) hipLaunchKernelGGL((conv_gemm_kernel<float, TILE_MT_BIG, 1, P>), grid, block, 0, s, a, M, KBn, n_tiles, ng, e);           \
        else if (c.big_n) hipLaunchKernelGGL((conv_gemm_kernel<float, 1, TILE_NT_BIG, P>), grid, block, 0, s, a, M, KBn, n_tiles, ng, e);           \
        else hipLaunchKernelGGL((conv_gemm_kernel<float, 1, 1, P>), grid, block, 0, s, a, M, KBn, n_tiles, ng, e);                                  \
    } while (0)
    if (a.ksize == 2) COSY_DGRAD_LAUNCH(GradPolicy<true>);
    else COSY_DGRAD_LAUNCH(GradPolicy<false>);
#undef COSY_DGRAD_LAUNCH
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

// what cosy_head_dgrad and cosy_head_wgrad ask of the layer's maps alike; -> the rows the levels hold, or -1 after set_error
long check_levels(const char* fn, const cosy_head_layer_t& a) {
    if (!(a.n_levels >= 1 && a.n_levels <= COSY_RPN_MAX_LEVELS)) { set_error("%s: n_levels=%d must lie in [1, %d]", fn, a.n_levels, COSY_RPN_MAX_LEVELS); return -1; }
    if (a.row_start[0] != 0) { set_error("%s: row_start[0]=%d must be 0", fn, a.row_start[0]); return -1; }
    for (int l = 0; l < a.n_levels; ++l) {
        if (!(a.H[l] >= 1 && a.W[l] >= 1 && (long)a.H[l] * a.W[l] <= HEAD_MAX_ROWS)) { set_error("%s: level %d is %d x %d cells", fn, l, a.H[l], a.W[l]); return -1; }
        const long n = (long)a.row_start[l + 1] - a.row_start[l];
        if (!(n >= 0 && n % ((long)a.H[l] * a.W[l]) == 0)) {
            set_error("%s: level %d owns %ld rows, not whole maps of %d x %d cells", fn, l, n, a.H[l], a.W[l]);
            return -1;
        }
    }
    const long M = a.row_start[a.n_levels];
    if (M > HEAD_MAX_ROWS) { set_error("%s: %ld rows exceed 2^30", fn, M); return -1; }
    return M;
}

}  // namespace
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
    hipStream_t s = (hipStream_t)stream;
    COSY_REQUIRE(ksize == 1 || ksize == 2 || ksize == 3, "cosy_head_weight_pack: ksize=%d must be 1, 3 or 2 (ConvTranspose2d(2, 2))", ksize);
    COSY_REQUIRE(c_in >= 8 && c_in % 8 == 0 && c_in <= (1 << 24), "cosy_head_weight_pack: the reduction length c_in=%d must be a positive multiple of 8", c_in);
    COSY_REQUIRE(n0 >= 1 && n1 >= 0 && (long)n0 + n1 <= (1 << 22), "cosy_head_weight_pack: n0=%d must be >= 1 and n1=%d >= 0", n0, n1);
    COSY_REQUIRE(ksize != 2 || (n1 == 0 && n0 % 8 == 0), "cosy_head_weight_pack: a deconvolution has no sibling and n0=%d a multiple of 8", n0);
    COSY_REQUIRE_PTR("cosy_head_weight_pack", w0); COSY_REQUIRE_PTR("cosy_head_weight_pack", b0);
    COSY_REQUIRE_PTR("cosy_head_weight_pack", fwd); COSY_REQUIRE_PTR("cosy_head_weight_pack", fwd_bias); COSY_REQUIRE_PTR("cosy_head_weight_pack", bwd);
    COSY_REQUIRE(n1 == 0 || (w1 != nullptr && b1 != nullptr), "cosy_head_weight_pack: null w1 or b1 with n1=%d", n1);
    const long O = n0 + n1, Nf = ksize == 2 ? 4 * O : O, Tf = ksize == 3 ? 9 : 1, Tb = ksize == 3 ? 9 : ksize == 2 ? 4 : 1;
    const long NPf = (Nf + 63) / 64 * 64, NPb = ((long)c_in + 63) / 64 * 64;
    const long n_fwd = NPf * Tf * ((c_in + 15) / 16 * 16), n_bwd = NPb * Tb * ((O + 15) / 16 * 16);
    const long total = n_fwd + n_bwd + NPf;
    COSY_REQUIRE(total <= (1L << 36), "cosy_head_weight_pack: %ld packed elements exceed 2^36", total);
    hipLaunchKernelGGL(head_weight_pack_kernel, dim3(cdiv(total, HEAD_THREADS)), dim3(HEAD_THREADS), 0, s, w0, b0, w1, b1, ksize, c_in, n0, n1, fwd, fwd_bias, bwd,
                       n_fwd, n_bwd, (int)NPf);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
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
    return launch_head_dgrad(a, (int)M, y, s);
}

int cosy_head_wgrad(const cosy_head_layer_t* layer, const float* g, float* dw0, float* db0, float* dw1, float* db1, void* workspace, size_t workspace_bytes,
                    cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
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
    const long n_out = (long)a.c_out * T * a.c_in + a.c_out;
    COSY_REQUIRE(n_out <= (1L << 36), "cosy_head_wgrad: c_out=%d x c_in=%d weights exceed 2^36", a.c_out, a.c_in);
    if (M == 0) {                                              // the gradient of an empty input: zeros of the right shape
        const long nw0 = (long)a.n_split * T * a.c_in, nw1 = (long)(a.c_out - a.n_split) * T * a.c_in;
        COSY_CHECK_HIP(hipMemsetAsync(dw0, 0, nw0 * sizeof(float), s));
        COSY_CHECK_HIP(hipMemsetAsync(db0, 0, (size_t)a.n_split * sizeof(float), s));
        if (nw1) {
            COSY_CHECK_HIP(hipMemsetAsync(dw1, 0, nw1 * sizeof(float), s));
            COSY_CHECK_HIP(hipMemsetAsync(db1, 0, (size_t)(a.c_out - a.n_split) * sizeof(float), s));
        }
        return COSY_OK;
    }
    COSY_REQUIRE_PTR("cosy_head_wgrad", a.x); COSY_REQUIRE_PTR("cosy_head_wgrad", g); COSY_REQUIRE_PTR("cosy_head_wgrad", workspace);
    const int slab = wgrad_slab_rows((int)M), nslab = cdiv(M, slab);
    const long slab_floats = wgrad_slab_floats(a.ksize, a.c_in, a.c_out);
    const size_t need = (size_t)nslab * (size_t)slab_floats * sizeof(float);
    COSY_REQUIRE(workspace_bytes >= need, "cosy_head_wgrad: workspace_bytes=%zu is less than the %zu bytes that %ld rows of c_in=%d, c_out=%d need "
                 "(cosy_head_wgrad_workspace_bytes)", workspace_bytes, need, M, a.c_in, a.c_out);
    const int GP = a.ksize == 2 ? a.c_out : pad8(a.c_out);
    const int o_tiles = cdiv(a.c_out, 16), c_groups = cdiv(a.c_in, a.ksize == 1 ? 64 : 16);
    const long n_waves = (long)o_tiles * c_groups;
    COSY_REQUIRE(n_waves <= 0x7fffffffL, "cosy_head_wgrad: c_out=%d x c_in=%d need more than 2^31 - 1 waves", a.c_out, a.c_in);
    const dim3 grid((unsigned)cdiv(n_waves, HEAD_THREADS / 64), (unsigned)nslab), block(HEAD_THREADS);
    float* partial = (float*)workspace;
    if (a.ksize == 1) hipLaunchKernelGGL(head_wgrad_kernel<0>, grid, block, 0, s, a, g, GP, (int)M, slab, (int)n_waves, c_groups, partial, slab_floats);
    else if (a.ksize == 3) hipLaunchKernelGGL(head_wgrad_kernel<1>, grid, block, 0, s, a, g, GP, (int)M, slab, (int)n_waves, c_groups, partial, slab_floats);
    else hipLaunchKernelGGL(head_wgrad_kernel<2>, grid, block, 0, s, a, g, GP, (int)M, slab, (int)n_waves, c_groups, partial, slab_floats);
    COSY_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(head_wgrad_combine_kernel, dim3(cdiv(n_out, HEAD_THREADS)), block, 0, s, partial, nslab, slab_floats, a.ksize, a.c_in, a.c_out, a.n_split,
                       dw0, db0, dw1, db1);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

}  // extern "C"
