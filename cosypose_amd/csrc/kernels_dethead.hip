// The detector's heads on the matrix pipe: every layer of Mask R-CNN's RPN head, box head + predictor and mask head +
// predictor is ONE implicit GEMM,  out[cout][pixel] = sum over (tap, channel) of w[cout][tap][channel] * x[pixel + tap][channel]:
//   * 3x3 conv (pad 1, stride 1): 9 taps; 1x1 conv: 1 tap; a linear layer: the 1x1 case on maps of one cell;
//   * ConvTranspose2d(k=2, s=2): a 1x1 GEMM to 4 C_out columns (o, dy, dx) whose epilogue scatters column (o, dy, dx) of cell (y, x) to (o, 2y+dy, 2x+dx).
// Activations are ROWS: row = (level, image, y, x) in that order, C_in contiguous channels of the storage type T (NHWC; a linear layer's row is
// its input vector).  cosy_head_pack makes rows out of a contiguous NCHW float32 map.  Weights arrive packed in fragment order (cosyhip.h).
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
// finite w.  Then ONE rounded bias add, then ReLU as torch's (x < 0 ? 0 : x: a NaN stays NaN), then the conversion to the store's type (round
// to nearest even).
// No atomics, no split-K: a wave owns its outputs from the first term to the store.  No LDS, no barriers: a wave past the last row leaves at once.
#include "net_device.h"

namespace cosy {
namespace {

constexpr int HEAD_THREADS = 256;            // 4 waves, stacked along the rows (pixels); every wave: 16 MT rows x 16 NT output channels
constexpr int HEAD_MT_BIG = 4, HEAD_NT_BIG = 4;
constexpr int HEAD_BIG_ROWS = 1024;          // M >= this: 64-row waves (256-row workgroups); below: 16-row waves (64-row workgroups)
constexpr int HEAD_BIG_TILES = 3;            // ceil(N / 16) >= this: 4 channel tiles per wave; below: 1
constexpr int HEAD_MAX_ROWS = 1 << 30;

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

template <typename T, int MT, int NT>
__global__ __launch_bounds__(HEAD_THREADS) void head_conv_kernel(const cosy_head_layer_t a, const int M, const int KBn, const int n_tiles, const int n_groups) {
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
    const int taps = a.ksize == 3 ? 9 : 1;
    const long S = (long)taps * KBn;                           // k-steps of one output

    // this lane's pixel of every row tile: the B operand's column and the result's column alike
    int r[MT], py[MT], px[MT], pH[MT], pW[MT], pb[MT], prs[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        r[mt] = row0 + mt * 16 + j;
        pH[mt] = 0; pW[mt] = 0; py[mt] = 0; px[mt] = 0; pb[mt] = 0; prs[mt] = 0;    // H = 0: no tap is inside, nothing is stored
        if (r[mt] < M) {
            int l = 0;
            while (l + 1 < a.n_levels && r[mt] >= a.row_start[l + 1]) ++l;
            const int H = a.H[l], W = a.W[l], rr = r[mt] - a.row_start[l];
            const int pix = rr % (H * W);
            pH[mt] = H; pW[mt] = W; prs[mt] = a.row_start[l];
            pb[mt] = rr / (H * W); py[mt] = pix / W; px[mt] = pix - py[mt] * W;
        }
    }

    f32x4 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int kb = 0; kb < KBn; ++kb) {
        for (int tap = 0; tap < taps; ++tap) {
            const int dy = taps == 9 ? tap / 3 - 1 : 0, dx = taps == 9 ? tap - (tap / 3) * 3 - 1 : 0;
            const long s = (long)tap * KBn + kb;
            frag_t xf[MT], wf[NT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const bool in = (unsigned)(py[mt] + dy) < (unsigned)pH[mt] && (unsigned)(px[mt] + dx) < (unsigned)pW[mt];
                xf[mt] = load_x<T>(x, in ? (long)(r[mt] + dy * pW[mt] + dx) * C_in : -1, kb, g, C_in);
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
        const int H = pH[mt], W = pW[mt], HW = H * W, pix = py[mt] * W + px[mt];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int col0 = (nt0 + nt) * 16 + 4 * g;
            if (nt0 + nt >= n_tiles || col0 >= N) continue;
            float v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                v[q] = acc[mt][nt][q] + bias[col0 + q];        // bias is padded like the weights
                if (a.relu) v[q] = relu_keep_nan(v[q]);
            }
            if (a.store == COSY_HEAD_STORE_ROWS) {             // N is a multiple of 8: the four channels exist
                put4((T*)a.out + (long)r[mt] * N + col0, v);
            } else if (a.store == COSY_HEAD_STORE_DECONV_ROWS || a.store == COSY_HEAD_STORE_DECONV_NCHW) {
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
    const int KBn = cdiv(a.c_in, DT<T>::KB), n_tiles = cdiv(a.c_out, 16);
    const bool big_m = M >= HEAD_BIG_ROWS, big_n = n_tiles >= HEAD_BIG_TILES;
    const int wg_rows = 64 * (big_m ? HEAD_MT_BIG : 1), nt = big_n ? HEAD_NT_BIG : 1;
    const long n_groups = cdiv(n_tiles, nt), blocks = (long)cdiv(M, wg_rows) * n_groups;
    COSY_REQUIRE(blocks <= 0x7fffffffL, "cosy_head_conv: %d rows x c_out=%d need more than 2^31 - 1 workgroups", M, a.c_out);
    const dim3 grid((unsigned)blocks);
    const int ng = (int)n_groups;
    if (big_m && big_n) hipLaunchKernelGGL((head_conv_kernel<T, HEAD_MT_BIG, HEAD_NT_BIG>), grid, dim3(HEAD_THREADS), 0, s, a, M, KBn, n_tiles, ng);
    else if (big_m) hipLaunchKernelGGL((head_conv_kernel<T, HEAD_MT_BIG, 1>), grid, dim3(HEAD_THREADS), 0, s, a, M, KBn, n_tiles, ng);
    else if (big_n) hipLaunchKernelGGL((head_conv_kernel<T, 1, HEAD_NT_BIG>), grid, dim3(HEAD_THREADS), 0, s, a, M, KBn, n_tiles, ng);
    else hipLaunchKernelGGL((head_conv_kernel<T, 1, 1>), grid, dim3(HEAD_THREADS), 0, s, a, M, KBn, n_tiles, ng);
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
