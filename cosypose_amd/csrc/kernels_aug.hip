// Training augmentations of the reference's PoseDataset.get_data (cosypose/datasets/pose_dataset.py:82-87, datasets/augmentations.py:40-125)
// on a collated uint8 batch, byte for byte what Pillow 12 gives: background paste, GaussianBlur(k), ImageEnhance Sharpness / Contrast /
// Brightness / Color, float32 grey.  DESIGN.md section 14 states the arithmetic; tests/aug_ref.py is its numpy twin.
//
// Three launches; the one dependency that spans a frame is Contrast's mean of L over the sharpened image:
//   aug_rows_kernel   paste + the three box passes along rows, on ROW_TY x ROW_TX tiles with a 9-pixel halo in LDS     images -> T1
//                     (an image whose gate is off is pasted straight into `out`, point by point, and the later launches skip it)
//   aug_cols_kernel   the three box passes along columns, SMOOTH and the sharpness blend on COL_TY x COL_TX tiles       T1 -> T2
//                     (halo: 10 rows, 1 column), and the integer sum of L per image (one 64-bit integer atomic per workgroup)
//   aug_point_kernel  contrast, brightness, colour, grey                                                               T2 -> out
// Every pass indexes with clamping in IMAGE coordinates, so a pass never sees a value computed at a position outside the frame; a tile
// position whose inputs left the tile holds garbage that the 3 (r + 1) <= 9 halo keeps away from the pixels written.
// Integer stages are exact in any order.  The float32 stages are written with one rounding per operation: the file is compiled with
// contraction off (the pragma below and -ffp-contract=off in build.FILE_FLAGS), a fused multiply-add gives other bytes.
#include "cosy_common.h"

#pragma clang fp contract(off)

namespace cosy {
namespace {

constexpr int AUG_THREADS = 256;
constexpr int AUG_HALO = 9;                                  // three passes of reach r + 1, r <= 2
constexpr int ROW_TX = 128, ROW_TY = 8, ROW_TW = ROW_TX + 2 * AUG_HALO;
constexpr int COL_TX = 64, COL_TY = 64, COL_TW = COL_TX + 2, COL_TH = COL_TY + 2 * (AUG_HALO + 1);
constexpr int COL_PER_THREAD = COL_TX * COL_TY / AUG_THREADS;
static_assert(COL_TX * COL_TY % AUG_THREADS == 0, "every thread owns the same number of tile pixels");

struct AugRec {
    int bg, flags, k;
    float sharpness, contrast, brightness, color;
};

// A record the kernels cannot serve (a background row outside the table, a blur radius outside 1..3) turns into "copy the image".
__device__ __forceinline__ AugRec aug_load(const cosy_aug_params_t* __restrict__ params, int b, int n_bg) {
    const cosy_aug_params_t p = params[b];
    AugRec r = {p.bg, p.flags, p.k, p.sharpness, p.contrast, p.brightness, p.color};
    const bool bad = p.bg < -1 || p.bg >= n_bg || ((p.flags & COSY_AUG_GATE) && (p.k < 1 || p.k > 3));
    if (bad) { r.bg = -1; r.flags = 0; }
    return r;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// Pillow's box pass weights for GaussianBlur(k): box radius sqrt(k*k*12/3 + 1)/2 - 0.5 in float32, ww = 2^24 / (2 radius + 1),
// fw = (2^24 - (2 r + 1) ww) / 2.  255 * ((2r+1) ww + 2 fw) + 2^23 < 2^32.
__device__ __forceinline__ void box_weights(int k, int& r, unsigned& ww, unsigned& fw) {
    r = k - 1;
    ww = k == 1 ? 11184811u : k == 2 ? 4473924u : 2876094u;
    fw = k == 1 ? 2796202u : k == 2 ? 1677722u : 1198373u;
}

// One box pass at position `pos` of a line that lives in LDS with `stride` bytes between neighbours.  `pos` is in image coordinates, `org`
// is the image coordinate of line element 0; [lo, hi] is the part of the image line that the tile holds (the frame [0, n - 1] cut with
// [org, org + len - 1], never empty), so one clamp serves both the frame's border rule and the tile's bounds.
__device__ __forceinline__ unsigned char box_at(const unsigned char* line, int stride, int pos, int org, int lo, int hi, int r, unsigned ww,
                                                unsigned fw) {
    unsigned acc = 0;
    for (int d = -r; d <= r; ++d) acc += line[(clampi(pos + d, lo, hi) - org) * stride];
    const unsigned far = (unsigned)line[(clampi(pos - r - 1, lo, hi) - org) * stride] + (unsigned)line[(clampi(pos + r + 1, lo, hi) - org) * stride];
    return (unsigned char)((acc * ww + far * fw + (1u << 23)) >> 24);
}

// ImagingBlend's byte: deg + f (im - deg), the product and the sum each rounded to float32, clipped, truncated.
__device__ __forceinline__ unsigned blend(int deg, int im, float f) {
    const float t = __fadd_rn((float)deg, __fmul_rn(f, (float)(im - deg)));
    return t <= 0.f ? 0u : t >= 255.f ? 255u : (unsigned)(int)t;
}

__device__ __forceinline__ unsigned luma_sum(unsigned r, unsigned g, unsigned b) { return r * 19595u + g * 38470u + b * 7471u; }
__device__ __forceinline__ unsigned luma(unsigned r, unsigned g, unsigned b) { return (luma_sum(r, g, b) + 0x8000u) >> 16; }

__global__ __launch_bounds__(AUG_THREADS) void aug_rows_kernel(const unsigned char* images, const unsigned char* __restrict__ masks,
                                                               const unsigned char* __restrict__ backgrounds, int n_bg,
                                                               const cosy_aug_params_t* __restrict__ params, int H, int W, unsigned char* t1,
                                                               unsigned char* out, unsigned long long* __restrict__ sum_l) {
    __shared__ unsigned char buf[2][ROW_TY * ROW_TW];
    const int b = blockIdx.z, x0 = blockIdx.x * ROW_TX, y0 = blockIdx.y * ROW_TY, tid = threadIdx.x;
    const AugRec rec = aug_load(params, b, n_bg);
    const size_t plane = (size_t)H * W;
    const unsigned char* im = images + (size_t)b * 3 * plane;
    const unsigned char* mk = rec.bg >= 0 ? masks + (size_t)b * plane : nullptr;
    const unsigned char* bg = rec.bg >= 0 ? backgrounds + (size_t)rec.bg * 3 * plane : nullptr;
    if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) sum_l[b] = 0;          // read by the next launch only
    if (!(rec.flags & COSY_AUG_GATE)) {                                        // paste only, each byte read and written by one thread
        unsigned char* o = out + (size_t)b * 3 * plane;
        for (int e = tid; e < ROW_TY * ROW_TX; e += AUG_THREADS) {
            const int y = y0 + e / ROW_TX, x = x0 + e % ROW_TX;
            if (y >= H || x >= W) continue;
            const size_t at = (size_t)y * W + x;
            const bool paste = mk && mk[at] == 0;
            for (int c = 0; c < 3; ++c) o[c * plane + at] = paste ? bg[c * plane + at] : im[c * plane + at];
        }
        return;
    }
    int r;
    unsigned ww, fw;
    box_weights(rec.k, r, ww, fw);
    unsigned char* o = t1 + (size_t)b * 3 * plane;
    const int lo = max(0, x0 - AUG_HALO), hi = min(W - 1, x0 - AUG_HALO + ROW_TW - 1);
    for (int c = 0; c < 3; ++c) {
        for (int e = tid; e < ROW_TY * ROW_TW; e += AUG_THREADS) {
            const int y = y0 + e / ROW_TW, x = clampi(x0 - AUG_HALO + e % ROW_TW, 0, W - 1);
            unsigned char v = 0;
            if (y < H) {
                const size_t at = (size_t)y * W + x;
                v = (mk && mk[at] == 0) ? bg[c * plane + at] : im[c * plane + at];
            }
            buf[0][e] = v;
        }
        __syncthreads();
        for (int pass = 0; pass < 3; ++pass) {
            const unsigned char* src = buf[pass & 1];
            unsigned char* dst = buf[(pass & 1) ^ 1];
            for (int e = tid; e < ROW_TY * ROW_TW; e += AUG_THREADS) {
                const int row = e / ROW_TW, x = x0 - AUG_HALO + e % ROW_TW;
                if (x >= 0 && x < W) dst[e] = box_at(src + row * ROW_TW, 1, x, x0 - AUG_HALO, lo, hi, r, ww, fw);
            }
            __syncthreads();
        }
        for (int e = tid; e < ROW_TY * ROW_TX; e += AUG_THREADS) {              // three passes: the result is in buf[1]
            const int row = e / ROW_TX, lx = e % ROW_TX, y = y0 + row, x = x0 + lx;
            if (y < H && x < W) o[c * plane + (size_t)y * W + x] = buf[1][row * ROW_TW + lx + AUG_HALO];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(AUG_THREADS) void aug_cols_kernel(const unsigned char* __restrict__ t1, int n_bg,
                                                               const cosy_aug_params_t* __restrict__ params, int H, int W,
                                                               unsigned char* __restrict__ t2, unsigned long long* sum_l) {
    __shared__ unsigned char buf[2][COL_TH * COL_TW];
    __shared__ unsigned wave_sum[AUG_THREADS / 64];
    const int b = blockIdx.z, x0 = blockIdx.x * COL_TX, y0 = blockIdx.y * COL_TY, tid = threadIdx.x;
    const AugRec rec = aug_load(params, b, n_bg);
    if (!(rec.flags & COSY_AUG_GATE)) return;
    int r;
    unsigned ww, fw;
    box_weights(rec.k, r, ww, fw);
    const size_t plane = (size_t)H * W;
    const unsigned char* in = t1 + (size_t)b * 3 * plane;
    unsigned char* o = t2 + (size_t)b * 3 * plane;
    const bool sharpen = (rec.flags & COSY_AUG_SHARPNESS) && H >= 3 && W >= 3;
    const int ty0 = y0 - (AUG_HALO + 1), tx0 = x0 - 1;                          // image coordinates of tile element (0, 0)
    const int lo = max(0, ty0), hi = min(H - 1, ty0 + COL_TH - 1);
    const float kf1 = 1.0f / 13.0f, kf5 = 5.0f / 13.0f;                         // float32(k) / float32(13), as Pillow stores its kernel
    unsigned lacc[COL_PER_THREAD];
#pragma unroll
    for (int i = 0; i < COL_PER_THREAD; ++i) lacc[i] = 0;
    for (int c = 0; c < 3; ++c) {
        for (int e = tid; e < COL_TH * COL_TW; e += AUG_THREADS) {
            const int y = clampi(ty0 + e / COL_TW, 0, H - 1), x = clampi(tx0 + e % COL_TW, 0, W - 1);
            buf[0][e] = in[c * plane + (size_t)y * W + x];
        }
        __syncthreads();
        for (int pass = 0; pass < 3; ++pass) {
            const unsigned char* src = buf[pass & 1];
            unsigned char* dst = buf[(pass & 1) ^ 1];
            for (int e = tid; e < COL_TH * COL_TW; e += AUG_THREADS) {
                const int col = e % COL_TW, y = ty0 + e / COL_TW;
                if (y >= 0 && y < H) dst[e] = box_at(src + col, COL_TW, y, ty0, lo, hi, r, ww, fw);
            }
            __syncthreads();
        }
        const unsigned char* bl = buf[1];                                       // the blurred channel
        const unsigned wl = c == 0 ? 19595u : c == 1 ? 38470u : 7471u;
#pragma unroll
        for (int i = 0; i < COL_PER_THREAD; ++i) {
            const int e = tid + i * AUG_THREADS, ly = e / COL_TX, lx = e % COL_TX, y = y0 + ly, x = x0 + lx;
            if (y >= H || x >= W) continue;
            const unsigned char* p = bl + (ly + AUG_HALO + 1) * COL_TW + lx + 1;
            unsigned v = p[0];
            if (sharpen && x >= 1 && x <= W - 2 && y >= 1 && y <= H - 2) {       // SMOOTH; the outermost rows and columns are copied
                float ss = 0.5f;
                for (int dy = 1; dy >= -1; --dy) {
                    const unsigned char* q = p + dy * COL_TW;
                    const float row = __fadd_rn(__fadd_rn(__fmul_rn((float)q[-1], kf1), __fmul_rn((float)q[0], dy == 0 ? kf5 : kf1)),
                                                __fmul_rn((float)q[1], kf1));
                    ss = __fadd_rn(ss, row);
                }
                const int deg = ss <= 0.f ? 0 : ss >= 255.f ? 255 : (int)ss;
                v = blend(deg, (int)v, rec.sharpness);
            }
            o[c * plane + (size_t)y * W + x] = (unsigned char)v;
            lacc[i] += v * wl;
        }
        __syncthreads();
    }
    if (!(rec.flags & COSY_AUG_CONTRAST)) return;
    unsigned sum = 0;
#pragma unroll
    for (int i = 0; i < COL_PER_THREAD; ++i) {
        const int e = tid + i * AUG_THREADS, y = y0 + e / COL_TX, x = x0 + e % COL_TX;
        if (y < H && x < W) sum += (lacc[i] + 0x8000u) >> 16;
    }
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
    if ((tid & 63) == 0) wave_sum[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) {
        unsigned total = 0;
        for (int w = 0; w < AUG_THREADS / 64; ++w) total += wave_sum[w];
        atomicAdd(&sum_l[b], (unsigned long long)total);                         // integer: the order of the workgroups does not matter
    }
}

// V pixels per thread (V = 4 when the planes are 4-byte aligned, else 1).
template <int V>
__global__ __launch_bounds__(AUG_THREADS) void aug_point_kernel(const unsigned char* __restrict__ t2, int n_bg,
                                                                const cosy_aug_params_t* __restrict__ params, long plane,
                                                                const unsigned long long* __restrict__ sum_l, unsigned char* __restrict__ out) {
    const int b = blockIdx.y;
    const AugRec rec = aug_load(params, b, n_bg);
    if (!(rec.flags & COSY_AUG_GATE)) return;
    const long at = ((long)blockIdx.x * AUG_THREADS + threadIdx.x) * V;
    if (at >= plane) return;
    const unsigned char* in = t2 + (size_t)b * 3 * plane + at;
    unsigned char* o = out + (size_t)b * 3 * plane + at;
    unsigned ch[3][V];
    for (int c = 0; c < 3; ++c) {
        if (V == 4) {
            const unsigned w = *reinterpret_cast<const unsigned*>(in + c * plane);
            for (int i = 0; i < V; ++i) ch[c][i] = (w >> (8 * i)) & 255u;
        } else {
            ch[c][0] = in[c * plane];
        }
    }
    int mean = 0;
    if (rec.flags & COSY_AUG_CONTRAST) {                                         // int(mean(L) + 0.5) = (2 sum + n) / (2 n)
        const unsigned long long n = (unsigned long long)plane;
        mean = (int)((2ull * sum_l[b] + n) / (2ull * n));
    }
#pragma unroll
    for (int i = 0; i < V; ++i) {
        unsigned r = ch[0][i], g = ch[1][i], bl = ch[2][i];
        if (rec.flags & COSY_AUG_CONTRAST) { r = blend(mean, r, rec.contrast); g = blend(mean, g, rec.contrast); bl = blend(mean, bl, rec.contrast); }
        if (rec.flags & COSY_AUG_BRIGHTNESS) { r = blend(0, r, rec.brightness); g = blend(0, g, rec.brightness); bl = blend(0, bl, rec.brightness); }
        if (rec.flags & COSY_AUG_COLOR) {
            const int l = (int)luma(r, g, bl);
            r = blend(l, r, rec.color); g = blend(l, g, rec.color); bl = blend(l, bl, rec.color);
        }
        if (rec.flags & COSY_AUG_GRAY) {                                          // 0.2989 R + 0.5870 G + 0.1140 B in float32, < 255
            const float gr = __fadd_rn(__fadd_rn(__fmul_rn(0.2989f, (float)r), __fmul_rn(0.5870f, (float)g)), __fmul_rn(0.1140f, (float)bl));
            r = g = bl = (unsigned)(int)gr;
        }
        ch[0][i] = r; ch[1][i] = g; ch[2][i] = bl;
    }
    for (int c = 0; c < 3; ++c) {
        if (V == 4) {
            *reinterpret_cast<unsigned*>(o + c * plane) = ch[c][0] | (ch[c][1] << 8) | (ch[c][2] << 16) | (ch[c][3] << 24);
        } else {
            o[c * plane] = (unsigned char)ch[c][0];
        }
    }
}

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
size_t aug_head_bytes(int B) { return align_up((size_t)B * sizeof(unsigned long long), 256); }
size_t aug_batch_bytes(int B, int H, int W) { return align_up((size_t)B * 3 * H * W, 256); }

}  // namespace
}  // namespace cosy

using namespace cosy;

extern "C" {

size_t cosy_augment_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return aug_head_bytes(B) + 2 * aug_batch_bytes(B, H, W);
}

int cosy_augment_batch(const unsigned char* images, const unsigned char* masks, const unsigned char* backgrounds, int n_bg,
                       const cosy_aug_params_t* params, int B, int H, int W, unsigned char* out, void* workspace, size_t workspace_bytes,
                       cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    COSY_REQUIRE(B >= 0 && H > 0 && W > 0 && n_bg >= 0, "cosy_augment_batch: B=%d H=%d W=%d n_bg=%d", B, H, W, n_bg);
    COSY_REQUIRE(B <= COSY_MAX_GRID_Y, "cosy_augment_batch: B=%d exceeds %d images per call", B, COSY_MAX_GRID_Y);
    COSY_REQUIRE(cdiv(H, ROW_TY) <= COSY_MAX_GRID_Y && (long)H * W < (1L << 31), "cosy_augment_batch: a frame of %d x %d is too large", H, W);
    if (B == 0) return COSY_OK;
    COSY_REQUIRE_PTR("cosy_augment_batch", images); COSY_REQUIRE_PTR("cosy_augment_batch", params);
    COSY_REQUIRE_PTR("cosy_augment_batch", out); COSY_REQUIRE_PTR("cosy_augment_batch", workspace);
    COSY_REQUIRE(n_bg == 0 || (masks && backgrounds), "cosy_augment_batch: n_bg=%d without masks or backgrounds", n_bg);
    COSY_REQUIRE(workspace_bytes >= cosy_augment_workspace_bytes(B, H, W), "cosy_augment_batch: workspace_bytes=%zu < %zu", workspace_bytes,
                 cosy_augment_workspace_bytes(B, H, W));
    COSY_REQUIRE(((uintptr_t)workspace & 15) == 0, "cosy_augment_batch: workspace not 16-byte aligned");
    unsigned long long* sum_l = (unsigned long long*)workspace;
    unsigned char* t1 = (unsigned char*)workspace + aug_head_bytes(B);
    unsigned char* t2 = t1 + aug_batch_bytes(B, H, W);
    const long plane = (long)H * W;
    hipLaunchKernelGGL(aug_rows_kernel, dim3(cdiv(W, ROW_TX), cdiv(H, ROW_TY), B), dim3(AUG_THREADS), 0, s, images, masks, backgrounds, n_bg, params,
                       H, W, t1, out, sum_l);
    COSY_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(aug_cols_kernel, dim3(cdiv(W, COL_TX), cdiv(H, COL_TY), B), dim3(AUG_THREADS), 0, s, t1, n_bg, params, H, W, t2, sum_l);
    COSY_CHECK_HIP(hipGetLastError());
    if (plane % 4 == 0 && ((uintptr_t)out & 3) == 0) {
        hipLaunchKernelGGL(aug_point_kernel<4>, dim3(cdiv(plane, 4L * AUG_THREADS), B), dim3(AUG_THREADS), 0, s, t2, n_bg, params, plane, sum_l, out);
    } else {
        hipLaunchKernelGGL(aug_point_kernel<1>, dim3(cdiv(plane, AUG_THREADS), B), dim3(AUG_THREADS), 0, s, t2, n_bg, params, plane, sum_l, out);
    }
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

}  // extern "C"
