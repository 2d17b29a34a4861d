// The trunk's data gradient as a template over the type of its rows (DESIGN.md sections 29 and 30): the forward GEMM's chain over the rows g
// with the transposed, tap-flipped weight, the parity classes of a stride-2 layer, and the store that adds up to two operands (SAME, EVEN,
// NEAREST_T), applies the ReLU mask of the layer below and converts ONCE to the rows' type.  kernels_detbwd.hip instantiates it for float32 rows
// (cosy_head_dgrad, cosy_trunk_dgrad) and for bfloat16 rows (cosy_trunk_dgrad16, and cosy_head_dgrad16, whose NCHW store writes the accumulator
// as float32).  Beside it, the host code both row types share wherever it launches no kernel of one file alone: the packing rules and their
// validator (kernels_detopt.hip's pack table runs both too), the gradient packs' validator, the level check and the data gradients' contracts.
//   float32 rows: every term of a block is one fmaf, four v_mfma_f32_16x16x4_f32 per (block of 16 o, live tap).
//   16-bit rows: one v_mfma_f32_16x16x32 per (block of 32 o, live tap); the products are exact in float32, the accumulation is float32.
// Store, per element: t = acc; t = t + (float)operand, in the order given, every + one rounded float32 add; t = y <= 0 ? +0.0 : t (a NaN y
// passes t); then one conversion to T (round to nearest even).  No atomics, no LDS: equal inputs give equal bits.
#pragma once
#include "dethead_device.h"

namespace cosy {
namespace detbwd {

using namespace headgemm;

inline int pad8(int n) { return (n + 7) / 8 * 8; }
inline bool aligned(const void* p, int bytes) { return ((uintptr_t)p & (uintptr_t)(bytes - 1)) == 0; }

// The first pass of a weight gradient as kernels_detbwd.hip's run_wgrad<T> planned it: the grid is (waves / 4, nslab).  The float32 rows' kernel
// lives in kernels_detbwd.hip, the bfloat16 rows' in kernels_detbwd16.hip; a wave takes 16 outputs x wgrad_group_channels<T>(ksize) channels.
struct wgrad_plan_t {
    int GP, M, slab, nslab, n_waves, c_groups, want_db;
    float* partial;
    long slab_floats;
};
template <typename T> constexpr int wgrad_group_channels(int ksize) { return ksize == 1 || (sizeof(T) == 2 && ksize == 2) ? 64 : 16; }
void launch_wgrad(const cosy_head_layer_t& a, int stride, const float* g, const wgrad_plan_t& p, hipStream_t s);
void launch_wgrad(const cosy_head_layer_t& a, int stride, const bf16_t* g, const wgrad_plan_t& p, hipStream_t s);

// the element (o, tap, c) of a layer's weight in torchvision's layout; o runs over the first tensor's outputs, then the second's.
// ksize 1 / 3: (O, C, k, k) or (O, C); ksize 2: ConvTranspose2d's (C, O, 2, 2)
__device__ __forceinline__ float weight_at(const float* __restrict__ w0, const float* __restrict__ w1, int ksize, int C, int n0, int n1, int o, int tap, int c) {
    if (ksize == 2) return w0[((long)c * n0 + o) * 4 + tap];
    const int T = ksize == 3 ? 9 : 1;
    return o < n0 ? w0[((long)o * C + c) * T + tap] : w1[((long)(o - n0) * C + c) * T + tap];
}

// The packing rules, stated once: cosy_head_weight_pack / cosy_trunk_weight_pack (T = float), their 16-bit forms (T = bf16_t) and the pack
// table's one launch (kernels_detopt.hip) all run this function, one thread per element i of [fwd | bwd | fwd_bias].
// Fragment order of cosy_head_conv, E = 16 / sizeof(T) elements per lane and KB = 4 E per block of the reduction: element [nt][tap][kb][lane][e]
// holds W[16 nt + (lane & 15)][tap][KB kb + E (lane >> 4) + e].
// forward: W = the layer's (rows o; ksize 2: rows (o, dy, dx), one tap), the host packing's bytes, and the bias or shift padded like it;
// backward: W = ws = w scale[o] rounded once to float32 (scale null: w), rows c, reduction o, taps flipped (ksize 3) or (dy, dx) (ksize 2).
// Siblings: w0 then w1; the trunk's layers are the case n1 = 0, b0 = shift.  The store converts ONCE to T (round to nearest even; float: none).
template <typename T> struct pack_frag { static constexpr int E_LOG2 = sizeof(T) == 4 ? 2 : 3, E = 1 << E_LOG2, KB = 4 * E; };

template <typename T>
__device__ __forceinline__ void weight_pack_element(const long i, const float* __restrict__ w0, const float* __restrict__ b0, const float* __restrict__ w1,
                                                    const float* __restrict__ b1, const float* __restrict__ scale, const int ksize, const int C, const int n0,
                                                    const int n1, T* __restrict__ fwd, float* __restrict__ fwd_bias, T* __restrict__ bwd, const long n_fwd,
                                                    const long n_bwd, const int n_bias) {
    constexpr int E_LOG2 = pack_frag<T>::E_LOG2, E = pack_frag<T>::E, KB = pack_frag<T>::KB;
    const int O = n0 + n1;
    if (i < n_fwd + n_bwd) {
        const bool back = i >= n_fwd;
        const long k = back ? i - n_fwd : i;
        const int taps = back ? (ksize == 3 ? 9 : ksize == 2 ? 4 : 1) : (ksize == 3 ? 9 : 1);
        const int N = back ? C : (ksize == 2 ? 4 * O : O), K = back ? O : C;           // rows and reduction length of this packing
        const int KBn = (K + KB - 1) / KB;
        const int e = (int)(k & (E - 1)), lane = (int)((k >> E_LOG2) & 63);
        const long s = k >> (E_LOG2 + 6);
        const int kb = (int)(s % KBn), tap = (int)((s / KBn) % taps), nt = (int)(s / ((long)KBn * taps));
        const int n = 16 * nt + (lane & 15), r = KB * kb + E * (lane >> 4) + e;
        float v = 0.f;
        if (n < N && r < K) {
            if (!back) v = ksize == 2 ? weight_at(w0, w1, 2, C, n0, n1, n >> 2, n & 3, r) : weight_at(w0, w1, ksize, C, n0, n1, n, tap, r);
            else {
                v = weight_at(w0, w1, ksize, C, n0, n1, r, ksize == 3 ? 8 - tap : tap, n);
                if (scale != nullptr) v = v * scale[r];
            }
        }
        (back ? bwd : fwd)[k] = (T)v;
    } else if (i < n_fwd + n_bwd + n_bias) {
        const int n = (int)(i - n_fwd - n_bwd);
        const int o = ksize == 2 ? n >> 2 : n;
        float v = 0.f;
        if (o < O) v = o < n0 ? b0[o] : b1[o - n0];
        fwd_bias[n] = v;
    }
}

// the elements of one layer's packings for a block of KB of the reduction (16: float32, 32: 16-bit): fwd, bwd, and the floats of fwd_bias
struct pack_sizes_t { long n_fwd, n_bwd, n_bias; };
inline pack_sizes_t pack_sizes(int ksize, int c_in, int n0, int n1, int KB) {
    const long O = (long)n0 + n1, Nf = ksize == 2 ? 4 * O : O, Tf = ksize == 3 ? 9 : 1, Tb = ksize == 3 ? 9 : ksize == 2 ? 4 : 1;
    const long NPf = (Nf + 63) / 64 * 64, NPb = ((long)c_in + 63) / 64 * 64;
    return pack_sizes_t{NPf * Tf * (((long)c_in + KB - 1) / KB * KB), NPb * Tb * ((O + KB - 1) / KB * KB), NPf};
}

// What every weight pack asks of its arguments, whoever packs: the four entry points (`at`: the entry's name) and every row of the pack table
// (`at`: "cosy_pack_table_build: layer l").  The trunk's layers are the case n1 = 0, b0 = shift.  KB: pack_frag<T>::KB of the packings' type.
// -> COSY_OK and the sizes of the packings, or COSY_EINVAL after set_error
inline int check_weight_pack(const char* at, const void* w0, const void* b0, const void* w1, const void* b1, const void* scale, const void* fwd, const void* fwd_bias,
                             const void* bwd, long long ksize, long long c_in, long long n0, long long n1, int KB, pack_sizes_t* sizes) {
    COSY_REQUIRE(ksize == 1 || ksize == 2 || ksize == 3, "%s: ksize=%lld must be 1, 3 or 2 (ConvTranspose2d(2, 2))", at, ksize);
    COSY_REQUIRE(c_in >= 8 && c_in % 8 == 0 && c_in <= (1 << 24), "%s: the reduction length c_in=%lld must be a positive multiple of 8", at, c_in);
    COSY_REQUIRE(n0 >= 1 && n1 >= 0 && n0 <= (1 << 22) && n1 <= (1 << 22) && n0 + n1 <= (1 << 22), "%s: n0=%lld must be >= 1 and n1=%lld >= 0", at, n0, n1);
    COSY_REQUIRE(ksize != 2 || (n1 == 0 && n0 % 8 == 0), "%s: a deconvolution has no sibling and n0=%lld a multiple of 8", at, n0);
    COSY_REQUIRE(scale == nullptr || (n1 == 0 && ksize != 2 && n0 % 8 == 0), "%s: a layer with a scale is one 1x1 or 3x3 convolution of a multiple of 8 outputs, got "
                 "ksize=%lld n0=%lld n1=%lld", at, ksize, n0, n1);
    COSY_REQUIRE(w0 != nullptr, "%s: null w0", at); COSY_REQUIRE(b0 != nullptr, "%s: null b0 (the bias, or the trunk's shift)", at);
    COSY_REQUIRE(fwd != nullptr, "%s: null fwd", at); COSY_REQUIRE(fwd_bias != nullptr, "%s: null fwd_bias", at); COSY_REQUIRE(bwd != nullptr, "%s: null bwd", at);
    COSY_REQUIRE(n1 == 0 || (w1 != nullptr && b1 != nullptr), "%s: null w1 or b1 with n1=%lld", at, n1);
    COSY_REQUIRE(aligned(w0, 4) && aligned(b0, 4) && aligned(w1, 4) && aligned(b1, 4) && aligned(scale, 4) && aligned(fwd_bias, 4) && aligned(fwd, 16) && aligned(bwd, 16),
                 "%s: the parameters, scale and fwd_bias must be 4-byte, fwd and bwd 16-byte aligned", at);
    *sizes = pack_sizes((int)ksize, (int)c_in, (int)n0, (int)n1, KB);
    const long total = sizes->n_fwd + sizes->n_bwd + sizes->n_bias;
    COSY_REQUIRE(total <= (1L << 36), "%s: %ld packed elements exceed 2^36", at, total);
    return COSY_OK;
}

// What both gradient packs (float32 rows: one thread per element; bfloat16 rows: eight columns per thread) ask of their arguments
// -> the elements of the rows (B HW GP; 0: nothing to do), or -1 after set_error
inline long check_grad_pack(const char* fn, const float* g0, const float* g1, const void* rows, int B, int n0, int n1, int HW) {
    if (!(B >= 0 && HW >= 1)) { set_error("%s: B=%d must be >= 0 and HW=%d >= 1", fn, B, HW); return -1; }
    if (!(n0 >= 0 && n1 >= 0 && n0 + n1 >= 1 && n0 + n1 <= (1 << 20))) { set_error("%s: n0=%d and n1=%d must be >= 0 and hold 1 to 2^20 columns", fn, n0, n1); return -1; }
    if ((long)B * HW > HEAD_MAX_ROWS) { set_error("%s: B HW = %ld rows exceed 2^30", fn, (long)B * HW); return -1; }
    if (B == 0) return 0;
    if (rows == nullptr) { set_error("%s: null rows", fn); return -1; }
    if (!(aligned(rows, 16) && aligned(g0, 4) && aligned(g1, 4))) { set_error("%s: rows must be 16-byte, g 4-byte aligned", fn); return -1; }
    const long total = (long)B * HW * pad8(n0 + n1);
    if (total > (1L << 38)) { set_error("%s: %ld elements exceed 2^38", fn, total); return -1; }
    return total;
}

// ConvTranspose2d(2, 2)'s data gradient on rows of T is dethead_device.h's conv_gemm_kernel over the transposed weight:
// the rows are the upstream gradient, no bias is added, and a row store may apply the ReLU mask of the layer below: y <= 0 ? +0.0 : v with y that
// layer's stored rows, in the rows' type (torch's threshold_backward: a NaN y passes v).  TAPS2: the four taps (dy, dx) = (0..1, 0..1) at stride 2,
// pad 0; the rows of the launch are the cells of the (H / 2, W / 2) map and no tap ever leaves the (H, W) map.
template <typename T> struct grad_epi_of { const T* y; };      // rows (M, c_out), or null
template <typename T> struct DeconvGradPolicyOf {
    static constexpr int STRIDE = 2;
    static constexpr bool TRUNK = false, GRAD = true, TAPS2 = true;
    typedef grad_epi_of<T> epi_t;
};

// M rows of the (H / 2, W / 2) maps, the four taps of the forward GEMM.  fn: the entry point the caller called; its name opens every message
template <typename T> int launch_deconv_dgrad(const char* fn, const cosy_head_layer_t& a, int M, const T* y, hipStream_t s) {
    typedef DeconvGradPolicyOf<T> P;
    const conv_grid_t c = conv_grid<T>(a, M);
    COSY_REQUIRE(c.blocks <= 0x7fffffffL, "%s: %d rows x c_out=%d need more than 2^31 - 1 workgroups", fn, M, a.c_out);
    const dim3 grid((unsigned)c.blocks), block(HEAD_THREADS);
    const grad_epi_of<T> e{y};
    if (c.big_m && c.big_n) hipLaunchKernelGGL((conv_gemm_kernel<T, TILE_MT_BIG, TILE_NT_BIG, P>), grid, block, 0, s, a, M, c.KBn, c.n_tiles, c.n_groups, e);
    else if (c.big_m) hipLaunchKernelGGL((conv_gemm_kernel<T, TILE_MT_BIG, 1, P>), grid, block, 0, s, a, M, c.KBn, c.n_tiles, c.n_groups, e);
    else if (c.big_n) hipLaunchKernelGGL((conv_gemm_kernel<T, 1, TILE_NT_BIG, P>), grid, block, 0, s, a, M, c.KBn, c.n_tiles, c.n_groups, e);
    else hipLaunchKernelGGL((conv_gemm_kernel<T, 1, 1, P>), grid, block, 0, s, a, M, c.KBn, c.n_tiles, c.n_groups, e);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

enum { ADD_NONE = 0, ADD_SAME = COSY_TRUNK_ADD_SAME, ADD_EVEN = COSY_TRUNK_ADD_EVEN, ADD_NEAREST_T = COSY_TRUNK_ADD_NEAREST_T };

template <typename T> struct tadd_t {
    const T* rows;                           // rows of c_out channels on maps of H x W per image
    int rule, H, W;
    float sy, sx;                            // NEAREST_T: (float)H_target / H, divided once on the host
};
template <typename T> struct tgrad_epi_t {
    const T* y;                              // rows on the dX grid, or null
    tadd_t<T> add[2];
    int par_y, par_x;                        // stride 2: the parity class of (iy, ix) this launch owns
};

// the finer cells [lo, hi) of one axis whose section 27 source cell is `cell`: nearest_src is monotone, so they are one contiguous range
__device__ __forceinline__ void nearest_range(int cell, float scale, int size, int fine, int& lo, int& hi) {
    int f = (int)((long)cell * fine / size);
    if (f > fine) f = fine;
    while (f > 0 && nearest_src(f - 1, scale, size) >= cell) --f;
    while (f < fine && nearest_src(f, scale, size) < cell) ++f;
    lo = f;
    while (f < fine && nearest_src(f, scale, size) == cell) ++f;
    hi = f;
}

template <typename T, int MT, int NT, int STRIDE>
__global__ __launch_bounds__(HEAD_THREADS) void dgrad_rows_kernel(const cosy_head_layer_t a, const int M, const int KBn, const int n_tiles, const int n_groups,
                                                                  const tgrad_epi_t<T> e) {
    typedef typename DT<T>::raw_t frag_t;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 15, g = lane >> 4;
    const unsigned total = gridDim.x, q8 = total / 8, rem = total % 8, xcd = blockIdx.x % 8, slot = blockIdx.x / 8;      // dethead_device.h's XCD remap
    const unsigned v = xcd * q8 + (xcd < rem ? xcd : rem) + slot;
    const int row0 = (int)((v / n_groups) * (HEAD_THREADS / 64) + wave) * 16 * MT;
    if (row0 >= M) return;                                     // wave-uniform
    const int nt0 = (int)(v % n_groups) * NT;
    const int O = a.c_in, N = a.c_out;                         // the reduction runs over the layer's outputs o; the result's columns are its inputs c
    const T* __restrict__ x = (const T*)a.x;
    const frag_t* __restrict__ w = (const frag_t*)a.w;
    const int taps = a.ksize == 3 ? 9 : 1;
    const long S = (long)taps * KBn;

    // this lane's cell of the dX grid: pH, pW its map (0: no such row), pb the image, py, px the cell, prs the level's first row
    int r[MT], py[MT], px[MT], pH[MT], pW[MT], pb[MT], prs[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        r[mt] = row0 + mt * 16 + j;
        pH[mt] = 0; pW[mt] = 0; py[mt] = 0; px[mt] = 0; pb[mt] = 0; prs[mt] = 0;
        if (r[mt] < M) {
            if constexpr (STRIDE == 1) {
                int l = 0;
                while (l + 1 < a.n_levels && r[mt] >= a.row_start[l + 1]) ++l;
                const int H = a.H[l], W = a.W[l], rr = r[mt] - a.row_start[l];
                const int pix = rr % (H * W);
                pH[mt] = H; pW[mt] = W; prs[mt] = a.row_start[l];
                pb[mt] = rr / (H * W); py[mt] = pix / W; px[mt] = pix - py[mt] * W;
            } else {                                           // one level; the rows are the cells of one parity class
                const int H = a.H[0], W = a.W[0], nY = (H + 1 - e.par_y) / 2, nX = (W + 1 - e.par_x) / 2;
                const int pix = r[mt] % (nY * nX), cy = pix / nX;
                pH[mt] = H; pW[mt] = W;
                pb[mt] = r[mt] / (nY * nX); py[mt] = 2 * cy + e.par_y; px[mt] = 2 * (pix - cy * nX) + e.par_x;
            }
        }
    }

    f32x4 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int kb = 0; kb < KBn; ++kb) {
        for (int tap = 0; tap < taps; ++tap) {
            const int ey = taps == 9 ? tap / 3 - 1 : 0, ex = taps == 9 ? tap - (tap / 3) * 3 - 1 : 0;      // g lives at the cell + (ey, ex)
            if constexpr (STRIDE == 2)
                if (((ey + e.par_y) & 1) || ((ex + e.par_x) & 1)) continue;                                // a dead tap of this class: no MFMA (wave-uniform)
            const long s = (long)tap * KBn + kb;
            frag_t xf[MT], wf[NT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                if constexpr (STRIDE == 1) {
                    const bool in = (unsigned)(py[mt] + ey) < (unsigned)pH[mt] && (unsigned)(px[mt] + ex) < (unsigned)pW[mt];
                    xf[mt] = load_x<T>(x, in ? (long)(r[mt] + ey * pW[mt] + ex) * O : -1, kb, g, O);
                } else {
                    const int Ho = (pH[mt] - 1) / 2 + 1, Wo = (pW[mt] - 1) / 2 + 1;
                    const int oy = (py[mt] + ey) >> 1, ox = (px[mt] + ex) >> 1;                            // py + ey is even and >= 0 for a live tap
                    const bool in = pH[mt] != 0 && oy < Ho && ox < Wo;
                    xf[mt] = load_x<T>(x, in ? (((long)pb[mt] * Ho + oy) * Wo + ox) * O : -1, kb, g, O);
                }
            }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) wf[nt] = nt0 + nt < n_tiles ? w[((long)(nt0 + nt) * S + s) * 64 + lane] : zero_frag<T>();
            if constexpr (sizeof(T) == 4) {
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
                        if (nt0 + nt < n_tiles)                // wave-uniform
#pragma unroll
                            for (int mt = 0; mt < MT; ++mt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[nt][t], xf[mt][t], acc[mt][nt], 0, 0, 0);
            } else {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    if (nt0 + nt < n_tiles)                    // wave-uniform
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt) mma(acc[mt][nt], wf[nt], xf[mt]);
            }
        }
    }

#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        if (pH[mt] == 0) continue;
        const int H = pH[mt], W = pW[mt], iy = py[mt], ix = px[mt];
        const long cell = (long)prs[mt] + ((long)pb[mt] * H + iy) * W + ix;                                // the row of the dX grid
        // the operands' rows of this cell: [lo, hi) ranges of the operand's grid, empty where the rule leaves the cell untouched
        int ylo[2], yhi[2], xlo[2], xhi[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            ylo[k] = yhi[k] = xlo[k] = xhi[k] = 0;
            const tadd_t<T>& ad = e.add[k];
            if (ad.rule == ADD_SAME) { ylo[k] = iy; yhi[k] = iy + 1; xlo[k] = ix; xhi[k] = ix + 1; }
            else if (ad.rule == ADD_EVEN) {
                if (!(iy & 1) && !(ix & 1)) { ylo[k] = iy >> 1; yhi[k] = ylo[k] + 1; xlo[k] = ix >> 1; xhi[k] = xlo[k] + 1; }
            } else if (ad.rule == ADD_NEAREST_T) {
                nearest_range(iy, ad.sy, H, ad.H, ylo[k], yhi[k]);
                nearest_range(ix, ad.sx, W, ad.W, xlo[k], xhi[k]);
            }
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int col0 = (nt0 + nt) * 16 + 4 * g;
            if (nt0 + nt >= n_tiles || col0 >= N) continue;
            float t[4] = {acc[mt][nt][0], acc[mt][nt][1], acc[mt][nt][2], acc[mt][nt][3]};
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const tadd_t<T>& ad = e.add[k];
                if (ad.rule == ADD_NONE) continue;
                for (int fy = ylo[k]; fy < yhi[k]; ++fy)
                    for (int fx = xlo[k]; fx < xhi[k]; ++fx) {
                        float rv[4];
                        load4(ad.rows + (((long)pb[mt] * ad.H + fy) * ad.W + fx) * N + col0, rv);
#pragma unroll
                        for (int q = 0; q < 4; ++q) t[q] = t[q] + rv[q];
                    }
            }
            if (e.y != nullptr) {
                float yv[4];
                load4(e.y + cell * N + col0, yv);
#pragma unroll
                for (int q = 0; q < 4; ++q) t[q] = yv[q] <= 0.f ? 0.f : t[q];
            }
            if (a.store == COSY_HEAD_STORE_ROWS) {
                put4((T*)a.out + cell * N + col0, t);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    ((float*)a.out)[(long)N * prs[mt] + (((long)pb[mt] * N + col0 + q) * H + iy) * W + ix] = t[q];
            }
        }
    }
}

// fn: the entry point the caller called; its name opens every message
template <typename T, int STRIDE> int launch_dgrad_rows(const char* fn, const cosy_head_layer_t& a, int M, const tgrad_epi_t<T>& e, hipStream_t s) {
    const conv_grid_t c = conv_grid<T>(a, M);
    COSY_REQUIRE(c.blocks <= 0x7fffffffL, "%s: %d rows x c_out=%d need more than 2^31 - 1 workgroups", fn, M, a.c_out);
    const dim3 grid((unsigned)c.blocks), block(HEAD_THREADS);
    if (c.big_m && c.big_n) hipLaunchKernelGGL((dgrad_rows_kernel<T, TILE_MT_BIG, TILE_NT_BIG, STRIDE>), grid, block, 0, s, a, M, c.KBn, c.n_tiles, c.n_groups, e);
    else if (c.big_m) hipLaunchKernelGGL((dgrad_rows_kernel<T, TILE_MT_BIG, 1, STRIDE>), grid, block, 0, s, a, M, c.KBn, c.n_tiles, c.n_groups, e);
    else if (c.big_n) hipLaunchKernelGGL((dgrad_rows_kernel<T, 1, TILE_NT_BIG, STRIDE>), grid, block, 0, s, a, M, c.KBn, c.n_tiles, c.n_groups, e);
    else hipLaunchKernelGGL((dgrad_rows_kernel<T, 1, 1, STRIDE>), grid, block, 0, s, a, M, c.KBn, c.n_tiles, c.n_groups, e);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

// what every entry point asks of the layer's maps alike; -> the rows the levels hold, or -1 after set_error
inline long check_levels(const char* fn, const cosy_head_layer_t& a) {
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

// cosy_trunk_dgrad's contract (cosyhip.h) on rows of T, after the caller's check of the layer pointer and of dtype: the argument checks, the
// operands' grids and the one launch (stride 1) or the four parity-class launches (stride 2)
template <typename T> int run_trunk_dgrad(const char* fn, const cosy_head_layer_t& a, int stride, const T* add0, int rule0, int add0_H, int add0_W, const T* add1,
                                          int rule1, int add1_H, int add1_W, const T* y, hipStream_t s) {
    COSY_REQUIRE(a.ksize == 1 || a.ksize == 3, "%s: ksize=%d must be 1 or 3", fn, a.ksize);
    COSY_REQUIRE(stride == 1 || stride == 2, "%s: stride=%d must be 1 or 2", fn, stride);
    COSY_REQUIRE(!(stride == 2 && a.ksize == 1), "%s: a 1x1 at stride 2 is a stride-1 launch on its OUTPUT grid whose rows enter through "
                 "COSY_TRUNK_ADD_EVEN, not a launch over the input grid", fn);
    COSY_REQUIRE(a.c_in >= 8 && a.c_in % 8 == 0, "%s: the reduction length c_in=%d (the layer's output channels) must be a positive multiple of 8", fn, a.c_in);
    COSY_REQUIRE(a.c_out >= 8 && a.c_out % 8 == 0, "%s: c_out=%d (the layer's input channels) must be a positive multiple of 8", fn, a.c_out);
    COSY_REQUIRE(a.store == COSY_HEAD_STORE_ROWS || (sizeof(T) == 4 && a.store == COSY_HEAD_STORE_NCHW),
                 sizeof(T) == 4 ? "%s: store=%d is not COSY_HEAD_STORE_ROWS or COSY_HEAD_STORE_NCHW" : "%s: store=%d is not COSY_HEAD_STORE_ROWS (16-bit rows have no NCHW store)",
                 fn, a.store);
    COSY_REQUIRE(a.relu == 0, "%s: relu=%d must be 0 (the mask is given by y)", fn, a.relu);
    COSY_REQUIRE(a.store != COSY_HEAD_STORE_NCHW || a.n_split == a.c_out, "%s: an NCHW store takes n_split == c_out=%d", fn, a.c_out);
    const long M_all = check_levels(fn, a);
    if (M_all < 0) return COSY_EINVAL;
    COSY_REQUIRE(stride == 1 || a.n_levels == 1, "%s: stride=2 takes one level, got n_levels=%d", fn, a.n_levels);
    const int H = a.H[0], W = a.W[0];
    const long B = M_all / ((long)H * W);                      // images of level 0 (the only level wherever B is used)
    tgrad_epi_t<T> e;
    e.y = y; e.par_y = 0; e.par_x = 0;
    const T* rows[2] = {add0, add1};
    const int rules[2] = {rule0, rule1}, aH[2] = {add0_H, add1_H}, aW[2] = {add0_W, add1_W};
    for (int k = 0; k < 2; ++k) {
        tadd_t<T>& ad = e.add[k];
        ad.rows = rows[k]; ad.rule = rules[k]; ad.H = aH[k]; ad.W = aW[k]; ad.sy = 1.f; ad.sx = 1.f;
        COSY_REQUIRE(ad.rule == ADD_NONE || ad.rule == ADD_SAME || ad.rule == ADD_EVEN || ad.rule == ADD_NEAREST_T,
                     "%s: add operand %d: rule=%d is not COSY_TRUNK_ADD_NONE, _SAME, _EVEN or _NEAREST_T", fn, k, ad.rule);
        if (ad.rule == ADD_NONE) { ad.rows = nullptr; ad.H = 1; ad.W = 1; continue; }
        COSY_REQUIRE(a.n_levels == 1, "%s: an add operand takes one level, got n_levels=%d", fn, a.n_levels);
        if (ad.rule == ADD_SAME) { ad.H = H; ad.W = W; }
        if (ad.rule == ADD_EVEN)
            COSY_REQUIRE(ad.H == (H - 1) / 2 + 1 && ad.W == (W - 1) / 2 + 1, "%s: add operand %d: an EVEN operand of %d x %d maps lives on %d x %d cells, got %d x %d",
                         fn, k, H, W, (H - 1) / 2 + 1, (W - 1) / 2 + 1, ad.H, ad.W);
        if (ad.rule == ADD_NEAREST_T) {
            COSY_REQUIRE(ad.H >= H && ad.W >= W && (long)ad.H * ad.W <= HEAD_MAX_ROWS, "%s: add operand %d: a NEAREST_T operand of %d x %d cells is coarser "
                         "than the target's %d x %d (or too large)", fn, k, ad.H, ad.W, H, W);
            COSY_REQUIRE(B * ad.H * ad.W <= HEAD_MAX_ROWS, "%s: add operand %d: its rows exceed 2^30", fn, k);
            ad.sy = (float)H / (float)ad.H; ad.sx = (float)W / (float)ad.W;
        }
    }
    if (M_all == 0) return COSY_OK;
    COSY_REQUIRE(a.x != nullptr && a.w != nullptr && a.out != nullptr, "%s: null layer->x, w or out", fn);
    for (int k = 0; k < 2; ++k) COSY_REQUIRE(e.add[k].rule == ADD_NONE || e.add[k].rows != nullptr, "%s: add operand %d: null rows with rule=%d", fn, k, e.add[k].rule);
    COSY_REQUIRE(((uintptr_t)a.x & 15) == 0 && ((uintptr_t)a.w & 15) == 0 && ((uintptr_t)a.out & 15) == 0 && ((uintptr_t)y & 15) == 0 && ((uintptr_t)add0 & 15) == 0 &&
                 ((uintptr_t)add1 & 15) == 0, "%s: x, w, out, y and the add operands must be 16-byte aligned", fn);
    if (stride == 1) return launch_dgrad_rows<T, 1>(fn, a, (int)M_all, e, s);
    for (int par = 0; par < 4; ++par) {                        // the four parity classes of (iy, ix): four row ranges, each with its fixed tap set
        e.par_y = par >> 1; e.par_x = par & 1;
        const long M = B * ((H + 1 - e.par_y) / 2) * ((W + 1 - e.par_x) / 2);
        if (M == 0) continue;
        const int rc = launch_dgrad_rows<T, 2>(fn, a, (int)M, e, s);
        if (rc != COSY_OK) return rc;
    }
    return COSY_OK;
}

// cosy_head_dgrad's contract (cosyhip.h) on rows of T, after the caller's check of the layer pointer and of dtype.  An NCHW store writes the
// accumulator as float32 whatever T is
template <typename T> int run_head_dgrad(const char* fn, const cosy_head_layer_t& a, const T* y, hipStream_t s) {
    COSY_REQUIRE(a.ksize == 1 || a.ksize == 2 || a.ksize == 3, "%s: ksize=%d must be 1, 3 or 2 (ConvTranspose2d(2, 2))", fn, a.ksize);
    COSY_REQUIRE(a.c_in >= 8 && a.c_in % 8 == 0, "%s: the reduction length c_in=%d must be a positive multiple of 8", fn, a.c_in);
    COSY_REQUIRE(a.c_out >= 8 && a.c_out % 8 == 0, "%s: c_out=%d (the layer's input channels) must be a positive multiple of 8", fn, a.c_out);
    COSY_REQUIRE(a.store == COSY_HEAD_STORE_ROWS || a.store == COSY_HEAD_STORE_NCHW, "%s: store=%d is not COSY_HEAD_STORE_ROWS or COSY_HEAD_STORE_NCHW", fn, a.store);
    COSY_REQUIRE(a.relu == 0, "%s: relu=%d must be 0 (the mask is given by y)", fn, a.relu);
    COSY_REQUIRE(a.store != COSY_HEAD_STORE_NCHW || (a.n_split == a.c_out && y == nullptr), "%s: an NCHW store takes n_split == c_out=%d and no y", fn, a.c_out);
    const long rows_in = check_levels(fn, a);
    if (rows_in < 0) return COSY_EINVAL;
    long M = rows_in;
    if (a.ksize == 2) {
        COSY_REQUIRE(a.n_levels == 1 && a.H[0] % 2 == 0 && a.W[0] % 2 == 0, "%s: ksize 2 takes one level of even maps, got %d levels of %d x %d", fn, a.n_levels, a.H[0],
                     a.W[0]);
        M = rows_in / 4;
    }
    if (M == 0) return COSY_OK;
    COSY_REQUIRE(a.x != nullptr && a.w != nullptr && a.out != nullptr, "%s: null layer->x, w or out", fn);
    COSY_REQUIRE(aligned(a.x, 16) && aligned(a.w, 16) && aligned(a.out, 16) && aligned(y, 16), "%s: x, w, out and y must be 16-byte aligned", fn);
    if (a.ksize == 2) return launch_deconv_dgrad<T>(fn, a, (int)M, y, s);
    const tadd_t<T> none{nullptr, ADD_NONE, 1, 1, 1.f, 1.f};
    return launch_dgrad_rows<T, 1>(fn, a, (int)M, tgrad_epi_t<T>{y, {none, none}, 0, 0}, s);
}

}  // namespace detbwd
}  // namespace cosy
