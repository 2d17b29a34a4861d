// The detector's optimiser step: torch.optim.SGD on flat float32 buffers, and the repack of every trainable layer's
// packings in ONE launch after it.
//   * sgd_step_kernel: d = g + wd w; m' = d (first step) or mu m + d; w' = w - lr m'.  Every product and every sum is one rounded float32
//     operation (this file is compiled without contraction, as kernels_dettrain.hip is); wd == 0 forms no product, mu == 0 touches no buffer:
//     both are template parameters, so a NaN or an Inf goes exactly where these operations carry it.  Streaming: a thread moves 16 bytes per
//     buffer and iteration, the grid (GRID_PER_CU workgroups per compute unit) strides over the body, the n % 4 last elements are the scalar
//     tail of the first threads.  64-bit offsets, no atomics, no LDS.
//   * pack_table_kernel: the per-layer packs of kernels_detbwd.hip, all layers in one grid.  The table (device memory,
//     built once) holds the first workgroup of every layer, then one pack_layer_t per layer; a workgroup finds its layer by a binary search of
//     the first column -- blockIdx.x alone decides, so every thread of the workgroup takes the same layer -- and runs detbwd_device.h's
//     weight_pack_element on its element: the packing rules exist once, and so do the checks of a row (check_weight_pack).
#include <cstdio>
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
        void* ptrs[8];                                    // w0, b0, w1, b1, scale, fwd, fwd_bias, bwd
        for (int k = 0; k < 8; ++k) ptrs[k] = (void*)(uintptr_t)r[k];
        const long long ksize = r[8], c_in = r[9], n0 = r[10], n1 = r[11], dtype = r[12];
        char at[48];                                      // opens every message of this row
        snprintf(at, sizeof at, "cosy_pack_table_build: layer %d", l);
        COSY_REQUIRE(dtype == COSY_F32 || dtype == COSY_BF16, "%s: dtype=%lld is not COSY_F32 or COSY_BF16 (float16 training needs a loss scaler, which is not built)", at,
                     dtype);
        pack_sizes_t z;                                   // the rest is what the per-layer packs check (detbwd_device.h)
        if (const int rc = check_weight_pack(at, ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptrs[4], ptrs[5], ptrs[6], ptrs[7], ksize, c_in, n0, n1,
                                             dtype == COSY_F32 ? pack_frag<float>::KB : pack_frag<bf16_t>::KB, &z))
            return rc;
        first[l] = wgs;
        wgs += (z.n_fwd + z.n_bwd + z.n_bias + HEAD_THREADS - 1) / HEAD_THREADS;
        layers[l] = pack_layer_t{(const float*)ptrs[0], (const float*)ptrs[1], n1 ? (const float*)ptrs[2] : nullptr, n1 ? (const float*)ptrs[3] : nullptr,
                                 (const float*)ptrs[4], ptrs[5], (float*)ptrs[6], ptrs[7], z.n_fwd, z.n_bwd, (int)ksize, (int)c_in, (int)n0, (int)n1, (int)dtype,
                                 (int)z.n_bias};
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
