// The detector's optimiser step: torch.optim.SGD on flat float32 buffers, and the repack of every trainable layer's
// packings in ONE launch after it.
//   * sgd_step_kernel: d = g + wd w; m' = d (first step) or mu m + d; w' = w - lr m'.  Every product and every sum is one rounded float32
//     operation (this file is compiled without contraction, as kernels_dettrain.hip is); wd == 0 forms no product, mu == 0 touches no buffer:
//     both are template parameters, so a NaN or an Inf goes exactly where these operations carry it.  Streaming: a thread moves 16 bytes per
//     buffer and iteration, the grid (GRID_PER_CU workgroups per compute unit) strides over the body, the n % 4 last elements are the scalar
//     tail of the first threads.  64-bit offsets, no atomics, no LDS.
//   * pack_table_kernel: the per-layer packs of kernels_detbwd.hip / kernels_detbwd16.hip, all layers in one grid.  The table (device memory,
//     built once) holds the first workgroup of every layer, then one pack_layer_t per layer; a workgroup finds its layer by a binary search of
//     the first column -- blockIdx.x alone decides, so every thread of the workgroup takes the same layer -- and runs detbwd_device.h's
//     weight_pack_element on its element: the packing rules exist once.
#include <vector>
#include "detbwd_device.h"

namespace cosy {
namespace {

using namespace headgemm;
using namespace detbwd;

constexpr int SGD_THREADS = 256, SGD_VEC = 4, GRID_PER_CU = 8;
constexpr int PACK_ROW_WORDS = 13, PACK_MAX_LAYERS = 4096;

template <bool WD, bool MOM>
__device__ __forceinline__ void sgd_element(float& w, const float g, float& m, const float lr, const float mu, const float wd, const bool first) {
    float d = g;
    if (WD) {
        const float decay = wd * w;
        d = g + decay;
    }
    float step = d;
    if (MOM) {
        if (!first) {
            const float kept = mu * m;
            step = kept + d;
        }
        m = step;
    }
    const float move = lr * step;
    w = w - move;
}

template <bool WD, bool MOM>
__global__ __launch_bounds__(SGD_THREADS) void sgd_step_kernel(float* __restrict__ params, const float* __restrict__ grads, float* __restrict__ mom, const long n,
                                                               const float lr, const float mu, const float wd, const int first_step) {
    const bool first = first_step != 0;
    const long n4 = n / SGD_VEC;
    const long tid = (long)blockIdx.x * SGD_THREADS + threadIdx.x, stride = (long)gridDim.x * SGD_THREADS;
    f32x4* __restrict__ p4 = (f32x4*)params;
    const f32x4* __restrict__ g4 = (const f32x4*)grads;
    f32x4* __restrict__ m4 = (f32x4*)mom;
    for (long i = tid; i < n4; i += stride) {
        f32x4 w = p4[i];
        const f32x4 g = g4[i];
        f32x4 m = f32x4{0.f, 0.f, 0.f, 0.f};
        if (MOM && !first) m = m4[i];
#pragma unroll
        for (int e = 0; e < SGD_VEC; ++e) {
            float we = w[e], me = m[e];
            sgd_element<WD, MOM>(we, g[e], me, lr, mu, wd, first);
            w[e] = we; m[e] = me;
        }
        if (MOM) m4[i] = m;
        p4[i] = w;
    }
    const long i = n4 * SGD_VEC + tid;               // the tail: at most three elements, the first threads of the grid
    if (i < n) {
        float w = params[i], m = 0.f;
        if (MOM && !first) m = mom[i];
        sgd_element<WD, MOM>(w, grads[i], m, lr, mu, wd, first);
        if (MOM) mom[i] = m;
        params[i] = w;
    }
}

// one layer of the pack table, as the kernel reads it
struct pack_layer_t {
    const float *w0, *b0, *w1, *b1, *scale;
    void* fwd;
    float* fwd_bias;
    void* bwd;
    long n_fwd, n_bwd;
    int ksize, c_in, n0, n1, dtype, n_bias;
};
static_assert(sizeof(pack_layer_t) % 8 == 0, "rows follow the first-workgroup column without padding");

inline size_t pack_first_bytes(int n_layers) { return ((size_t)(n_layers + 1) * sizeof(long) + 15) / 16 * 16; }
inline size_t pack_table_bytes(int n_layers) { return pack_first_bytes(n_layers) + (size_t)n_layers * sizeof(pack_layer_t); }

__global__ __launch_bounds__(HEAD_THREADS) void pack_table_kernel(const long* __restrict__ first, const pack_layer_t* __restrict__ layers, const int n_layers) {
    const long wg = blockIdx.x;
    int lo = 0, hi = n_layers;                       // first[lo] <= wg < first[hi]: first[0] = 0, first[n_layers] = the grid
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first[mid] <= wg) lo = mid; else hi = mid;
    }
    const pack_layer_t& L = layers[lo];
    const long i = (wg - first[lo]) * HEAD_THREADS + threadIdx.x;
    if (L.dtype == COSY_F32)
        weight_pack_element<float>(i, L.w0, L.b0, L.w1, L.b1, L.scale, L.ksize, L.c_in, L.n0, L.n1, (float*)L.fwd, L.fwd_bias, (float*)L.bwd, L.n_fwd, L.n_bwd, L.n_bias);
    else
        weight_pack_element<bf16_t>(i, L.w0, L.b0, L.w1, L.b1, L.scale, L.ksize, L.c_in, L.n0, L.n1, (bf16_t*)L.fwd, L.fwd_bias, (bf16_t*)L.bwd, L.n_fwd, L.n_bwd,
                                    L.n_bias);
}

int sgd_grid(int* blocks) {
    int dev = 0, cus = 0;
    COSY_CHECK_HIP(hipGetDevice(&dev));
    COSY_CHECK_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    COSY_REQUIRE(cus >= 1, "cosy_sgd_step: the device reports %d compute units", cus);
    *blocks = cus * GRID_PER_CU;
    return COSY_OK;
}

}  // namespace
}  // namespace cosy

using namespace cosy;

extern "C" {

long long cosy_sgd_step_pass_elements(void) {
    int blocks = 0;
    if (sgd_grid(&blocks) != COSY_OK) return 0;
    return (long long)blocks * SGD_THREADS * SGD_VEC;
}

int cosy_sgd_step(float* params, const float* grads, float* momentum_buf, long long n, float lr, float momentum, float weight_decay, int first_step,
                  cosy_stream_t stream) {
    COSY_REQUIRE(n >= 0 && n <= (1LL << 40), "cosy_sgd_step: n=%lld must be in [0, 2^40]", n);
    if (n == 0) return COSY_OK;
    COSY_REQUIRE_PTR("cosy_sgd_step", params); COSY_REQUIRE_PTR("cosy_sgd_step", grads);
    COSY_REQUIRE(momentum == 0.f || momentum_buf != nullptr, "cosy_sgd_step: null momentum_buf with momentum=%g", (double)momentum);
    COSY_REQUIRE(((uintptr_t)params & 15) == 0 && ((uintptr_t)grads & 15) == 0 && (momentum == 0.f || ((uintptr_t)momentum_buf & 15) == 0),
                 "cosy_sgd_step: params, grads and momentum_buf must be 16-byte aligned");
    int blocks = 0;
    if (const int rc = sgd_grid(&blocks)) return rc;
    const long need = ((long)n / SGD_VEC + SGD_THREADS - 1) / SGD_THREADS;      // a buffer shorter than one pass takes the workgroups it fills
    const dim3 grid((unsigned)(need < 1 ? 1 : need < blocks ? need : blocks)), block(SGD_THREADS);
    hipStream_t s = (hipStream_t)stream;
    const bool wd = weight_decay != 0.f, mom = momentum != 0.f;
#define COSY_SGD_LAUNCH(WD, MOM) hipLaunchKernelGGL((sgd_step_kernel<WD, MOM>), grid, block, 0, s, params, grads, momentum_buf, (long)n, lr, momentum, weight_decay, first_step)
    if (wd && mom) COSY_SGD_LAUNCH(true, true);
    else if (wd) COSY_SGD_LAUNCH(true, false);
    else if (mom) COSY_SGD_LAUNCH(false, true);
    else COSY_SGD_LAUNCH(false, false);
#undef COSY_SGD_LAUNCH
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

size_t cosy_pack_table_bytes(int n_layers) { return n_layers >= 1 && n_layers <= PACK_MAX_LAYERS ? pack_table_bytes(n_layers) : 0; }

int cosy_pack_table_build(const long long* rows, int n_layers, void* table, size_t table_bytes, long long* n_workgroups, cosy_stream_t stream) {
    COSY_REQUIRE(n_layers >= 1 && n_layers <= PACK_MAX_LAYERS, "cosy_pack_table_build: n_layers=%d must be in [1, %d]", n_layers, PACK_MAX_LAYERS);
    COSY_REQUIRE_PTR("cosy_pack_table_build", rows); COSY_REQUIRE_PTR("cosy_pack_table_build", table); COSY_REQUIRE_PTR("cosy_pack_table_build", n_workgroups);
    COSY_REQUIRE(((uintptr_t)table & 15) == 0, "cosy_pack_table_build: table must be 16-byte aligned");
    const size_t bytes = pack_table_bytes(n_layers);
    COSY_REQUIRE(table_bytes >= bytes, "cosy_pack_table_build: table_bytes=%zu is less than cosy_pack_table_bytes(%d)=%zu", table_bytes, n_layers, bytes);
    std::vector<unsigned char> host(bytes, 0);
    long* first = (long*)host.data();
    pack_layer_t* layers = (pack_layer_t*)(host.data() + pack_first_bytes(n_layers));
    long wgs = 0;
    for (int l = 0; l < n_layers; ++l) {
        const long long* r = rows + (size_t)l * PACK_ROW_WORDS;
        const uintptr_t w0 = (uintptr_t)r[0], b0 = (uintptr_t)r[1], w1 = (uintptr_t)r[2], b1 = (uintptr_t)r[3], scale = (uintptr_t)r[4], fwd = (uintptr_t)r[5],
                        fwd_bias = (uintptr_t)r[6], bwd = (uintptr_t)r[7];
        const long long ksize = r[8], c_in = r[9], n0 = r[10], n1 = r[11], dtype = r[12];
#define COSY_ROW "cosy_pack_table_build: layer %d: "
        COSY_REQUIRE(dtype == COSY_F32 || dtype == COSY_BF16, COSY_ROW "dtype=%lld is not COSY_F32 or COSY_BF16 (float16 training needs a loss scaler, which is not built)", l, dtype);
        COSY_REQUIRE(ksize == 1 || ksize == 2 || ksize == 3, COSY_ROW "ksize=%lld must be 1, 3 or 2 (ConvTranspose2d(2, 2))", l, ksize);
        COSY_REQUIRE(c_in >= 8 && c_in % 8 == 0 && c_in <= (1 << 24), COSY_ROW "the reduction length c_in=%lld must be a positive multiple of 8", l, c_in);
        COSY_REQUIRE(n0 >= 1 && n1 >= 0 && n0 <= (1 << 22) && n1 <= (1 << 22) && n0 + n1 <= (1 << 22), COSY_ROW "n0=%lld must be >= 1 and n1=%lld >= 0", l, n0, n1);
        COSY_REQUIRE(ksize != 2 || (n1 == 0 && n0 % 8 == 0), COSY_ROW "a deconvolution has no sibling and n0=%lld a multiple of 8", l, n0);
        COSY_REQUIRE(scale == 0 || (n1 == 0 && ksize != 2 && n0 % 8 == 0), COSY_ROW "a layer with a scale is one 1x1 or 3x3 convolution of a multiple of 8 outputs, got ksize=%lld n0=%lld n1=%lld",
                     l, ksize, n0, n1);
        COSY_REQUIRE(w0 != 0, COSY_ROW "null w0", l); COSY_REQUIRE(b0 != 0, COSY_ROW "null b0", l);
        COSY_REQUIRE(fwd != 0, COSY_ROW "null fwd", l); COSY_REQUIRE(fwd_bias != 0, COSY_ROW "null fwd_bias", l); COSY_REQUIRE(bwd != 0, COSY_ROW "null bwd", l);
        COSY_REQUIRE(n1 == 0 || (w1 != 0 && b1 != 0), COSY_ROW "null w1 or b1 with n1=%lld", l, n1);
        COSY_REQUIRE((w0 & 3) == 0 && (b0 & 3) == 0 && (w1 & 3) == 0 && (b1 & 3) == 0 && (scale & 3) == 0 && (fwd & 15) == 0 && (bwd & 15) == 0 && (fwd_bias & 3) == 0,
                     COSY_ROW "the parameters, scale and fwd_bias must be 4-byte, fwd and bwd 16-byte aligned", l);
        const pack_sizes_t z = pack_sizes((int)ksize, (int)c_in, (int)n0, (int)n1, dtype == COSY_F32 ? pack_frag<float>::KB : pack_frag<bf16_t>::KB);
        const long total = z.n_fwd + z.n_bwd + z.n_bias;
        COSY_REQUIRE(total <= (1L << 36), COSY_ROW "%ld packed elements exceed 2^36", l, total);
#undef COSY_ROW
        first[l] = wgs;
        wgs += (total + HEAD_THREADS - 1) / HEAD_THREADS;
        layers[l] = pack_layer_t{(const float*)w0, (const float*)b0, n1 ? (const float*)w1 : nullptr, n1 ? (const float*)b1 : nullptr, (const float*)scale, (void*)fwd,
                                 (float*)fwd_bias, (void*)bwd, z.n_fwd, z.n_bwd, (int)ksize, (int)c_in, (int)n0, (int)n1, (int)dtype, (int)z.n_bias};
    }
    first[n_layers] = wgs;
    COSY_REQUIRE(wgs <= 0x7fffffffL, "cosy_pack_table_build: the %d layers need %ld workgroups, more than 2^31 - 1", n_layers, wgs);
    hipStream_t s = (hipStream_t)stream;
    COSY_CHECK_HIP(hipMemcpyAsync(table, host.data(), bytes, hipMemcpyHostToDevice, s));
    COSY_CHECK_HIP(hipStreamSynchronize(s));             // `host` leaves with this call
    *n_workgroups = wgs;
    return COSY_OK;
}

int cosy_pack_table_run(const void* table, int n_layers, long long n_workgroups, cosy_stream_t stream) {
    COSY_REQUIRE(n_layers >= 1 && n_layers <= PACK_MAX_LAYERS, "cosy_pack_table_run: n_layers=%d must be in [1, %d]", n_layers, PACK_MAX_LAYERS);
    COSY_REQUIRE_PTR("cosy_pack_table_run", table);
    COSY_REQUIRE(n_workgroups >= 1 && n_workgroups <= 0x7fffffffLL, "cosy_pack_table_run: n_workgroups=%lld must be in [1, 2^31 - 1]", n_workgroups);
    const long* first = (const long*)table;
    const pack_layer_t* layers = (const pack_layer_t*)((const unsigned char*)table + pack_first_bytes(n_layers));
    hipLaunchKernelGGL(pack_table_kernel, dim3((unsigned)n_workgroups), dim3(HEAD_THREADS), 0, (hipStream_t)stream, first, layers, n_layers);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

}  // extern "C"
