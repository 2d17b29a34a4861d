// The implicit GEMM of the detector's layers, stated once (DESIGN.md sections 26 and 27): kernels_dethead.hip instantiates it for the heads
// (stride 1, bias + ReLU), kernels_dettrunk.hip for the ResNet trunk and the FPN (stride 1 or 2, scale / shift, residual, ReLU).  The policy is a
// compile-time type: the heads' instantiation holds no instruction of the trunk's stride or epilogue.
//
// The weights are the A operand of the MFMA and the pixels the B operand, so the result tile has its PIXEL on the lane (column = lane & 15)
// and four consecutive output channels in the lane's registers (row = 4 (lane >> 4) + reg): an NCHW store is 16 neighbouring pixels per
// register, a row store is four neighbouring channels per lane.
//
// Summation order of one output (stated in DESIGN.md section 26, restated by tests/dethead_ref.py): accumulator +0.0; the channels in blocks of
// KB (16 for float32, 32 for the 16-bit types) ascending; inside a block the taps (ky, kx) ascending; inside a tap the block's channels: float32
// in the order 4 g + t with t = 0..3 outside and g = 0..3 inside (0, 4, 8, 12, 1, 5, ...: a lane group loads four contiguous channels and MFMA t
// takes its t-th), every term one fmaf (v_mfma_f32_16x16x4_f32 is that chain, four channels per instruction); 16-bit: one v_mfma_f32_16x16x32 per
// (block, tap), products exact in float32, the order of the 32 additions inside the instruction is the hardware's and the same on every call.
// Blocks outside, taps inside: the nine taps of a block re-read the same 32 or 64 bytes of each neighbouring cell, which then come from the L1.
// A border tap and the channels past C_in in the last block are fed as +0.0 against the real / zero-padded weight: fma(0, w, acc) = acc for
// finite w; the address of a tap outside the map is never formed.
// Epilogue, heads: ONE rounded bias add, then ReLU as torch's (x < 0 ? 0 : x: a NaN stays NaN), then the conversion to the store's type (round
// to nearest even).  Trunk: fmaf(acc, scale, bias) (or the bias add without a scale), one rounded add of the residual, ReLU, the conversion.
// No atomics, no split-K: a wave owns its outputs from the first term to the store.  No LDS, no barriers: a wave past the last row leaves at once.
#pragma once
#include <type_traits>
#include "net_device.h"

namespace cosy {
namespace headgemm {

constexpr int HEAD_THREADS = 256;            // 4 waves, stacked along the rows (pixels); every wave: 16 MT rows x 16 NT output channels
constexpr int TILE_MT_BIG = 4, TILE_NT_BIG = 4;
constexpr int TILE_BIG_ROWS = 1024;          // M >= this: 64-row waves (256-row workgroups); below: 16-row waves (64-row workgroups)
constexpr int TILE_BIG_TILES = 3;            // ceil(N / 16) >= this: 4 channel tiles per wave; below: 1
constexpr int HEAD_MAX_ROWS = 1 << 30;

// what the trunk's epilogue reads beside the layer; the heads pass an empty one
struct no_epi_t {};
struct conv_epi_t {
    const float* scale;                      // c_out padded like bias, or null
    const void* residual;                    // rows (B res_H res_W, c_out) of the storage type, or null
    int res_H, res_W;
    float sy, sx;                            // (float)res_H / Ho, (float)res_W / Wo, divided once on the host
};

// STRIDE: 1, or 2 (one level only: the rows of the launch are the OUTPUT cells).  TRUNK: the scale / residual epilogue and no deconvolution store
template <int STRIDE_, bool TRUNK_> struct ConvPolicy {
    static constexpr int STRIDE = STRIDE_;
    static constexpr bool TRUNK = TRUNK_;
    static constexpr bool GRAD = false, TAPS2 = false;
    typedef typename std::conditional<TRUNK_, conv_epi_t, no_epi_t>::type epi_t;
};
typedef ConvPolicy<1, false> HeadPolicy;

// (A third policy, with GRAD and TAPS2 set, is detbwd_device.h's DeconvGradPolicyOf<T>: the data gradient of ConvTranspose2d(2, 2).)

template <typename T> __device__ __forceinline__ typename DT<T>::raw_t zero_frag() {
    typename DT<T>::raw_t z;
#pragma unroll
    for (int i = 0; i < DT<T>::EPL; ++i) z[i] = (T)0.f;
    return z;
}

// the pixel operand of one k-block: lane group g = lane >> 4 holds the contiguous channels kb KB + (KB / 4) g + (0 .. KB / 4 - 1), one 16-byte load
// (float32: element t feeds MFMA t of the block, which therefore sums the channels 4 g + t, g = 0..3); base < 0: the tap lies outside the map
template <typename T> __device__ __forceinline__ typename DT<T>::raw_t load_x(const T* __restrict__ x, long base, int kb, int g, int C_in) {
    typename DT<T>::raw_t v = zero_frag<T>();
    const int c = kb * DT<T>::KB + DT<T>::EPL * g;             // C_in is a multiple of 8: the lane's channels exist together or not at all
    if (base >= 0 && c < C_in) v = *(const typename DT<T>::raw_t*)(x + base + c);
    return v;
}

__device__ __forceinline__ float relu_keep_nan(float v) { return v < 0.f ? 0.f : v; }

__device__ __forceinline__ void put4(float* p, const float* v) { *(f32x4*)p = f32x4{v[0], v[1], v[2], v[3]}; }
__device__ __forceinline__ void put4(f16_t* p, const float* v) { *(f16x4*)p = f16x4{(f16_t)v[0], (f16_t)v[1], (f16_t)v[2], (f16_t)v[3]}; }
__device__ __forceinline__ void put4(bf16_t* p, const float* v) { *(bf16x4*)p = bf16x4{(bf16_t)v[0], (bf16_t)v[1], (bf16_t)v[2], (bf16_t)v[3]}; }

// torch's legacy mode='nearest' source index: min(floor(dst * scale), size - 1), the product in float32
__device__ __forceinline__ int nearest_src(int dst, float scale, int size) {
    const int s = (int)floorf((float)dst * scale);
    return s < size - 1 ? s : size - 1;
}

// the kernel itself is the template (not a body inlined into two kernels): hipcc schedules the heads' instantiation exactly as it did before the
// trunk existed only when the layer is the kernel's own by-value argument and the __restrict__ pointers are the kernel's own locals
template <typename T, int MT, int NT, typename P>
__global__ __launch_bounds__(HEAD_THREADS) void conv_gemm_kernel(const cosy_head_layer_t a, const int M, const int KBn, const int n_tiles, const int n_groups,
                                                                 const typename P::epi_t e) {
    typedef typename DT<T>::raw_t frag_t;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 15, g = lane >> 4;
    // Workgroups are handed to the 8 XCDs round-robin; the remap gives every XCD one contiguous run of (row tile, channel group) pairs, channel
    // groups fastest, so the workgroups that read the same cells -- the other channel groups, the row tiles above and below -- share an L2.
    // A bijection of [0, gridDim.x) for any grid size; placement changes speed only.
    const unsigned total = gridDim.x, q = total / 8, rem = total % 8, xcd = blockIdx.x % 8, slot = blockIdx.x / 8;
    const unsigned v = xcd * q + (xcd < rem ? xcd : rem) + slot;
    const int row0 = (int)((v / n_groups) * (HEAD_THREADS / 64) + wave) * 16 * MT;
    if (row0 >= M) return;                                     // wave-uniform
    const int nt0 = (int)(v % n_groups) * NT;
    const int C_in = a.c_in, N = a.c_out;
    const T* __restrict__ x = (const T*)a.x;
    const frag_t* __restrict__ w = (const frag_t*)a.w;
    const int taps = P::TAPS2 ? 4 : a.ksize == 3 ? 9 : 1;
    const long S = (long)taps * KBn;                           // k-steps of one output

    // this lane's pixel of every row tile: the B operand's column and the result's column alike.  pH, pW: the INPUT map (the taps' bounds);
    // py, px: the OUTPUT cell, which with stride 1 is the input cell of the centre tap
    int r[MT], py[MT], px[MT], pH[MT], pW[MT], pb[MT], prs[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        r[mt] = row0 + mt * 16 + j;
        pH[mt] = 0; pW[mt] = 0; py[mt] = 0; px[mt] = 0; pb[mt] = 0; prs[mt] = 0;    // H = 0: no tap is inside, nothing is stored
        if (r[mt] < M) {
            if constexpr (P::STRIDE == 1) {
                int l = 0;
                while (l + 1 < a.n_levels && r[mt] >= a.row_start[l + 1]) ++l;
                const int H = a.H[l], W = a.W[l], rr = r[mt] - a.row_start[l];
                const int pix = rr % (H * W);
                pH[mt] = H; pW[mt] = W; prs[mt] = a.row_start[l];
                pb[mt] = rr / (H * W); py[mt] = pix / W; px[mt] = pix - py[mt] * W;
            } else {                                           // one level; the rows are the output cells of (Ho, Wo) maps
                const int H = a.H[0], W = a.W[0], Ho = (H - 1) / P::STRIDE + 1, Wo = (W - 1) / P::STRIDE + 1;
                const int pix = r[mt] % (Ho * Wo);
                pH[mt] = H; pW[mt] = W;
                pb[mt] = r[mt] / (Ho * Wo); py[mt] = pix / Wo; px[mt] = pix - py[mt] * Wo;
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
            const int dy = P::TAPS2 ? tap >> 1 : taps == 9 ? tap / 3 - 1 : 0, dx = P::TAPS2 ? tap & 1 : taps == 9 ? tap - (tap / 3) * 3 - 1 : 0;
            const long s = (long)tap * KBn + kb;
            frag_t xf[MT], wf[NT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                if constexpr (P::STRIDE == 1) {
                    const bool in = (unsigned)(py[mt] + dy) < (unsigned)pH[mt] && (unsigned)(px[mt] + dx) < (unsigned)pW[mt];
                    xf[mt] = load_x<T>(x, in ? (long)(r[mt] + dy * pW[mt] + dx) * C_in : -1, kb, g, C_in);
                } else {
                    const int iy = P::STRIDE * py[mt] + dy, ix = P::STRIDE * px[mt] + dx;
                    const bool in = (unsigned)iy < (unsigned)pH[mt] && (unsigned)ix < (unsigned)pW[mt];
                    xf[mt] = load_x<T>(x, in ? (((long)pb[mt] * pH[mt] + iy) * pW[mt] + ix) * C_in : -1, kb, g, C_in);
                }
            }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) wf[nt] = nt0 + nt < n_tiles ? w[((long)(nt0 + nt) * S + s) * 64 + lane] : zero_frag<T>();
            if constexpr (sizeof(T) == 4) {                    // consecutive MFMAs go to different accumulators; every output still sums t = 0..3 in order
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

    const float* __restrict__ bias = a.bias;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        if (pH[mt] == 0) continue;
        // the OUTPUT map of this pixel
        const int H = P::STRIDE == 1 ? pH[mt] : (pH[mt] - 1) / P::STRIDE + 1, W = P::STRIDE == 1 ? pW[mt] : (pW[mt] - 1) / P::STRIDE + 1;
        const int HW = H * W, pix = py[mt] * W + px[mt];
        long res_row = 0;
        if constexpr (P::TRUNK)
            if (e.residual != nullptr)
                res_row = ((long)pb[mt] * e.res_H + nearest_src(py[mt], e.sy, e.res_H)) * e.res_W + nearest_src(px[mt], e.sx, e.res_W);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int col0 = (nt0 + nt) * 16 + 4 * g;
            if (nt0 + nt >= n_tiles || col0 >= N) continue;
            float v[4];
            if constexpr (P::TRUNK) {
                float res[4] = {0.f, 0.f, 0.f, 0.f};
                if (e.residual != nullptr) load4((const T*)e.residual + res_row * N + col0, res);      // a residual has c_out a multiple of 8
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    v[q] = e.scale != nullptr ? __builtin_fmaf(acc[mt][nt][q], e.scale[col0 + q], bias[col0 + q]) : acc[mt][nt][q] + bias[col0 + q];
                    if (e.residual != nullptr) v[q] = v[q] + res[q];
                    if (a.relu) v[q] = relu_keep_nan(v[q]);
                }
            } else if constexpr (P::GRAD) {
                float yv[4] = {1.f, 1.f, 1.f, 1.f};
                if (a.store == COSY_HEAD_STORE_ROWS && e.y != nullptr) load4(e.y + (long)r[mt] * N + col0, yv);
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = yv[q] <= 0.f ? 0.f : acc[mt][nt][q];
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    v[q] = acc[mt][nt][q] + bias[col0 + q];    // bias is padded like the weights
                    if (a.relu) v[q] = relu_keep_nan(v[q]);
                }
            }
            if (a.store == COSY_HEAD_STORE_ROWS) {             // N is a multiple of 8: the four channels exist
                put4((T*)a.out + (long)r[mt] * N + col0, v);
            } else if (!P::TRUNK && !P::GRAD && (a.store == COSY_HEAD_STORE_DECONV_ROWS || a.store == COSY_HEAD_STORE_DECONV_NCHW)) {
                const int o = col0 >> 2, Co = N >> 2;          // the lane's four columns: (o, dy, dx), dy, dx = 0, 1
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const long oy = 2 * py[mt] + (q >> 1), ox = 2 * px[mt] + (q & 1);
                    if (a.store == COSY_HEAD_STORE_DECONV_ROWS)
                        ((T*)a.out)[(4L * prs[mt] + ((long)pb[mt] * 2 * H + oy) * 2 * W + ox) * Co + o] = (T)v[q];
                    else
                        ((float*)a.out)[4L * prs[mt] * Co + (((long)pb[mt] * Co + o) * 2 * H + oy) * 2 * W + ox] = v[q];
                }
            } else {                                           // NCHW float32, columns [0, n_split) to out, the rest to out1
                const int n0 = a.n_split, n1 = N - a.n_split;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int col = col0 + q;
                    if (col >= N) break;
                    if (col < n0) ((float*)a.out)[(long)n0 * prs[mt] + ((long)pb[mt] * n0 + col) * HW + pix] = v[q];
                    else ((float*)a.out1)[(long)n1 * prs[mt] + ((long)pb[mt] * n1 + (col - n0)) * HW + pix] = v[q];
                }
            }
        }
    }
}

// the launch geometry both instantiations share: the tile goes by the rows M the launch OWNS (output cells) and by the channel tiles
struct conv_grid_t { bool big_m, big_n; int KBn, n_tiles, n_groups; long blocks; };
template <typename T> inline conv_grid_t conv_grid(const cosy_head_layer_t& a, int M) {
    conv_grid_t c;
    c.KBn = cdiv(a.c_in, DT<T>::KB); c.n_tiles = cdiv(a.c_out, 16);
    c.big_m = M >= TILE_BIG_ROWS; c.big_n = c.n_tiles >= TILE_BIG_TILES;
    const int wg_rows = 64 * (c.big_m ? TILE_MT_BIG : 1), nt = c.big_n ? TILE_NT_BIG : 1;
    c.n_groups = cdiv(c.n_tiles, nt);
    c.blocks = (long)cdiv(M, wg_rows) * c.n_groups;
    return c;
}

}  // namespace headgemm
}  // namespace cosy
