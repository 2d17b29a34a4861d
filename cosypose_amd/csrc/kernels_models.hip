// Object models: the BOP diameter (largest distance between two vertices, the toolkit's calc_pts_diameter), the axis-aligned box and
// the count of non-finite coordinates of a ragged batch of models in one call.  DESIGN.md section 20 holds the contract.
//
// The diameter is O(V^2) work on O(V) data.  The vertex pairs of a model are cut into square tiles of MI_TILE x MI_TILE vertices over
// the upper triangle (diagonal tiles included); the tiles of all models form one list with 64-bit indices, and the workgroups of one
// grid walk it.  A workgroup keeps the tile's column block in LDS as float64 and its row block in registers, two rows per thread, so a
// vertex is read from memory once per tile and every pair costs arithmetic only.
//
// The value is bit-equal to SciPy's cdist: dx = x_i - x_j in float64 (float32 input is widened first, which is exact), then
// ((dx dx + dy dy) + dz dz) with every operation rounded on its own -- this file is compiled with -ffp-contract=off, and the matrix form
// |a|^2 + |b|^2 - 2 a.b rounds differently, which rules the matrix pipe out.  The square root is the caller's, on the host.
//
// The pair: of all (i, j), i < j, that attain the maximum, the lexicographically smallest.  A thread walks j upwards for a fixed i and
// replaces on `>` only; threads, waves and tiles are then merged with ONE total order (larger s, then smaller i, then smaller j), so the
// result does not depend on which workgroup took which tile: every tile leaves its winner in the workspace with plain stores, and the
// last kernel merges a model's tiles.  No floating-point atomics, no atomics at all.
#include "reduce_device.h"

namespace cosy {

constexpr int MI_TILE = 512;          // tile edge in vertices: 256 threads x 2 rows; cosypose_amd/model_info.py TILE mirrors it
constexpr int MI_MAX_GRID = 1 << 15;  // workgroups of the pair kernel; a longer tile list is walked with this stride

struct MiBest {   // a candidate pair, 16 bytes; none: s = -1 (a real pair has s >= 0 or NaN, and a NaN never replaces anything)
    double s;
    int i, j;
};

__device__ __forceinline__ bool mi_better(const MiBest& a, const MiBest& b) {
    return a.s > b.s || (a.s == b.s && (a.i < b.i || (a.i == b.i && a.j < b.j)));
}

__device__ __forceinline__ MiBest mi_wave_best(MiBest v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        MiBest w;
        w.s = __shfl_xor(v.s, o, 64);
        w.i = __shfl_xor(v.i, o, 64);
        w.j = __shfl_xor(v.j, o, 64);
        if (mi_better(w, v)) v = w;
    }
    return v;
}

// the best of the 256 threads, in every thread; `scratch` = 4 entries of LDS
__device__ __forceinline__ MiBest mi_block_best(MiBest v, MiBest* scratch) {
    v = mi_wave_best(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    MiBest b = scratch[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
        if (mi_better(scratch[w], b)) b = scratch[w];
    return b;
}

__host__ __device__ static inline long long mi_tiles_of(long long V) {
    const long long nt = (V + MI_TILE - 1) / MI_TILE;
    return nt * (nt + 1) / 2;
}

// tile_start[m] = number of tiles before model m, tile_start[n] = total, from the DEVICE offsets.  A model whose offsets are not
// 0 <= offsets[m] <= offsets[m + 1] <= total_verts with fewer than 2^31 vertices gets no tiles (and no vertex of it is ever read).
__device__ __forceinline__ long long mi_model_verts(const long long* __restrict__ offsets, int m, long long total_verts) {
    const long long a = offsets[m], b = offsets[m + 1];
    return (a >= 0 && b >= a && b <= total_verts && b - a < (1LL << 31)) ? b - a : -1;
}

__global__ __launch_bounds__(256) void mi_plan_kernel(const long long* __restrict__ offsets, int n, long long total_verts, long long cap_tiles,
                                                      long long* __restrict__ tile_start) {
    __shared__ long long part[256];
    const int tid = threadIdx.x, run = (n + 255) / 256;
    const int m0 = min(n, tid * run), m1 = min(n, m0 + run);
    long long sum = 0;
    for (int m = m0; m < m1; ++m) sum += mi_tiles_of(max(mi_model_verts(offsets, m, total_verts), 0LL));
    part[tid] = sum;
    __syncthreads();
    long long at = 0;
    for (int t = 0; t < tid; ++t) at += part[t];
    for (int m = m0; m < m1; ++m) {
        tile_start[m] = min(at, cap_tiles);      // never past the partials the caller's workspace holds
        at += mi_tiles_of(max(mi_model_verts(offsets, m, total_verts), 0LL));
    }
    if (tid == 255) tile_start[n] = min(at, cap_tiles);
}

// the model of a tile: the last m with tile_start[m] <= t (models without tiles share their successor's start)
__device__ __forceinline__ int mi_model_of(const long long* __restrict__ tile_start, int n, long long t) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tile_start[mid] <= t) lo = mid; else hi = mid;
    }
    return lo;
}

// tile u of a model, column-major over the upper triangle: u = c (c + 1) / 2 + r with r <= c.  c by bisection in integers.
__device__ __forceinline__ void mi_tile_rc(long long u, int nt, int* r, int* c) {
    long long lo = 0, hi = nt;                   // c in [lo, hi)
    while (hi - lo > 1) {
        const long long mid = (lo + hi) >> 1;
        if (mid * (mid + 1) / 2 <= u) lo = mid; else hi = mid;
    }
    *c = (int)lo;
    *r = (int)(u - lo * (lo + 1) / 2);
}

template <typename T>
__global__ __launch_bounds__(256) void mi_pairs_kernel(const T* __restrict__ verts, const long long* __restrict__ offsets, int n, long long total_verts,
                                                       const long long* __restrict__ tile_start, MiBest* __restrict__ partial) {
    __shared__ double xs[MI_TILE], ys[MI_TILE], zs[MI_TILE];
    __shared__ MiBest scratch[4];
    const int tid = threadIdx.x;
    const long long total = tile_start[n];
    for (long long t = blockIdx.x; t < total; t += gridDim.x) {
        const int m = mi_model_of(tile_start, n, t);
        const long long V = mi_model_verts(offsets, m, total_verts);      // > 0: the model has tiles
        const T* __restrict__ p = verts + 3 * offsets[m];
        int r, c;
        mi_tile_rc(t - tile_start[m], (int)((V + MI_TILE - 1) / MI_TILE), &r, &c);
        const long long i0 = (long long)r * MI_TILE, j0 = (long long)c * MI_TILE;
        const int nj = (int)min((long long)MI_TILE, V - j0);
        __syncthreads();                         // the previous tile's column block is no longer read
        for (int k = tid; k < nj; k += 256) {
            xs[k] = (double)p[3 * (j0 + k)];
            ys[k] = (double)p[3 * (j0 + k) + 1];
            zs[k] = (double)p[3 * (j0 + k) + 2];
        }
        // two rows per thread; a row past the end of the model reads vertex V - 1 and is dropped below
        const long long ia = i0 + tid, ib = i0 + tid + 256;
        const long long la = min(ia, V - 1), lb = min(ib, V - 1);
        const double ax = (double)p[3 * la], ay = (double)p[3 * la + 1], az = (double)p[3 * la + 2];
        const double bx = (double)p[3 * lb], by = (double)p[3 * lb + 1], bz = (double)p[3 * lb + 2];
        __syncthreads();
        double sa = -1.0, sb = -1.0;
        int ja = 0, jb = 0;
        if (r != c) {
#pragma unroll 4
            for (int k = 0; k < nj; ++k) {
                const double x = xs[k], y = ys[k], z = zs[k];
                const double dxa = ax - x, dya = ay - y, dza = az - z;
                const double dxb = bx - x, dyb = by - y, dzb = bz - z;
                const double qa = (dxa * dxa + dya * dya) + dza * dza;
                const double qb = (dxb * dxb + dyb * dyb) + dzb * dzb;
                if (qa > sa) { sa = qa; ja = k; }
                if (qb > sb) { sb = qb; jb = k; }
            }
        } else {
            // a diagonal tile: only j > i.  (i0 == j0: the local numbers compare as the global ones do.)
#pragma unroll 4
            for (int k = 0; k < nj; ++k) {
                const double x = xs[k], y = ys[k], z = zs[k];
                const double dxa = ax - x, dya = ay - y, dza = az - z;
                const double dxb = bx - x, dyb = by - y, dzb = bz - z;
                const double qa = (dxa * dxa + dya * dya) + dza * dza;
                const double qb = (dxb * dxb + dyb * dyb) + dzb * dzb;
                if (k > tid && qa > sa) { sa = qa; ja = k; }
                if (k > tid + 256 && qb > sb) { sb = qb; jb = k; }
            }
        }
        MiBest a{ia < V ? sa : -1.0, (int)ia, (int)(j0 + ja)}, b{ib < V ? sb : -1.0, (int)ib, (int)(j0 + jb)};
        if (mi_better(b, a)) a = b;
        a = mi_block_best(a, scratch);
        if (tid == 0) partial[t] = a;
    }
}

// One workgroup per model: merges the model's tile winners, walks its vertices once for the box and the non-finite count, and writes the
// model's record in full.
template <typename T>
__global__ __launch_bounds__(256) void mi_final_kernel(const T* __restrict__ verts, const long long* __restrict__ offsets, int n, long long total_verts,
                                                       const long long* __restrict__ tile_start, const MiBest* __restrict__ partial,
                                                       cosy_model_info_t* __restrict__ out) {
    __shared__ MiBest scratch[4];
    __shared__ double lo_s[4][3], hi_s[4][3];
    __shared__ long long bad_s[4];
    const int m = blockIdx.x, tid = threadIdx.x;
    const long long V = mi_model_verts(offsets, m, total_verts);
    MiBest best{-1.0, 0x7fffffff, 0x7fffffff};
    for (long long t = tile_start[m] + tid; t < tile_start[m + 1]; t += 256) {
        const MiBest v = partial[t];
        if (mi_better(v, best)) best = v;
    }
    best = mi_block_best(best, scratch);
    const double inf = __builtin_inf();
    double lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    long long bad = 0;
    if (V > 0) {
        const T* __restrict__ p = verts + 3 * offsets[m];
        for (long long v = tid; v < V; v += 256) {
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const double x = (double)p[3 * v + d];
                bad += !(fabs(x) < inf);         // NaN and +-inf
                lo[d] = fmin(lo[d], x);
                hi[d] = fmax(hi[d], x);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        bad += __shfl_xor(bad, o, 64);
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            lo[d] = fmin(lo[d], __shfl_xor(lo[d], o, 64));
            hi[d] = fmax(hi[d], __shfl_xor(hi[d], o, 64));
        }
    }
    if ((tid & 63) == 0) {
        bad_s[tid >> 6] = bad;
#pragma unroll
        for (int d = 0; d < 3; ++d) { lo_s[tid >> 6][d] = lo[d]; hi_s[tid >> 6][d] = hi[d]; }
    }
    __syncthreads();
    if (tid == 0) {
        cosy_model_info_t o;
        const bool none = !(best.s >= 0.0);      // a single vertex (or no valid model): no pair
        o.s_max = none ? 0.0 : best.s;
        o.i = none ? 0 : best.i;
        o.j = none ? 0 : best.j;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            o.min[d] = fmin(fmin(lo_s[0][d], lo_s[1][d]), fmin(lo_s[2][d], lo_s[3][d]));
            o.max[d] = fmax(fmax(hi_s[0][d], hi_s[1][d]), fmax(hi_s[2][d], hi_s[3][d]));
        }
        o.n_bad = V > 0 ? ((bad_s[0] + bad_s[1]) + bad_s[2]) + bad_s[3] : -1;
        out[m] = o;
    }
}

static size_t mi_head_bytes(int n) { return (((size_t)n + 1) * sizeof(long long) + 15) / 16 * 16; }

// total tiles of the host offsets, or -1 where they are not a ragged batch of models of 1 .. 2^31 - 1 vertices
static long long mi_host_tiles(const long long* host_offsets, int n) {
    if (!host_offsets || host_offsets[0] < 0) return -1;
    long long total = 0;
    for (int m = 0; m < n; ++m) {
        const long long V = host_offsets[m + 1] - host_offsets[m];
        if (V < 1 || V >= (1LL << 31)) return -1;
        total += mi_tiles_of(V);
    }
    return total;
}

}  // namespace cosy

using namespace cosy;

extern "C" {

size_t cosy_model_info_workspace_bytes(const long long* host_offsets, int n) {
    if (n <= 0) return 0;
    const long long tiles = mi_host_tiles(host_offsets, n);
    return tiles < 0 ? 0 : mi_head_bytes(n) + (size_t)tiles * sizeof(MiBest);
}

int cosy_model_info(const void* verts, int elem_bytes, const long long* offsets, const long long* host_offsets, int n, cosy_model_info_t* out,
                    void* workspace, size_t workspace_bytes, cosy_stream_t stream) {
    static_assert(sizeof(MiBest) == 16 && sizeof(cosy_model_info_t) == 72, "layout of the partials and of the record");
    COSY_REQUIRE(n >= 0, "cosy_model_info: n=%d", n);
    if (n == 0) return COSY_OK;
    COSY_REQUIRE(elem_bytes == 4 || elem_bytes == 8, "cosy_model_info: elem_bytes=%d (4: float32, 8: float64)", elem_bytes);
    COSY_REQUIRE_PTR("cosy_model_info", verts); COSY_REQUIRE_PTR("cosy_model_info", offsets);
    COSY_REQUIRE_PTR("cosy_model_info", host_offsets); COSY_REQUIRE_PTR("cosy_model_info", out);
    COSY_REQUIRE_PTR("cosy_model_info", workspace);
    const long long tiles = mi_host_tiles(host_offsets, n);
    COSY_REQUIRE(tiles >= 0, "cosy_model_info: host_offsets must start at >= 0 and give every model 1 to 2^31 - 1 vertices");
    COSY_REQUIRE(((uintptr_t)verts & (elem_bytes - 1)) == 0, "cosy_model_info: verts not aligned to its %d-byte elements", elem_bytes);
    COSY_REQUIRE(((uintptr_t)out & 7) == 0, "cosy_model_info: out not 8-byte aligned");
    COSY_REQUIRE(workspace_bytes >= cosy_model_info_workspace_bytes(host_offsets, n), "cosy_model_info: workspace_bytes=%zu < %zu", workspace_bytes,
                 cosy_model_info_workspace_bytes(host_offsets, n));
    COSY_REQUIRE(((uintptr_t)workspace & 15) == 0, "cosy_model_info: workspace not 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    long long* tile_start = (long long*)workspace;
    MiBest* partial = (MiBest*)((char*)workspace + mi_head_bytes(n));
    const long long total_verts = host_offsets[n];
    hipLaunchKernelGGL(mi_plan_kernel, dim3(1), dim3(256), 0, s, offsets, n, total_verts, tiles, tile_start);
    COSY_CHECK_HIP(hipGetLastError());
    const unsigned grid = (unsigned)(tiles < MI_MAX_GRID ? tiles : MI_MAX_GRID);
    if (elem_bytes == 4) {
        hipLaunchKernelGGL(mi_pairs_kernel<float>, dim3(grid), dim3(256), 0, s, (const float*)verts, offsets, n, total_verts, (const long long*)tile_start,
                           partial);
        COSY_CHECK_HIP(hipGetLastError());
        hipLaunchKernelGGL(mi_final_kernel<float>, dim3(n), dim3(256), 0, s, (const float*)verts, offsets, n, total_verts, (const long long*)tile_start,
                           (const MiBest*)partial, out);
    } else {
        hipLaunchKernelGGL(mi_pairs_kernel<double>, dim3(grid), dim3(256), 0, s, (const double*)verts, offsets, n, total_verts,
                           (const long long*)tile_start, partial);
        COSY_CHECK_HIP(hipGetLastError());
        hipLaunchKernelGGL(mi_final_kernel<double>, dim3(n), dim3(256), 0, s, (const double*)verts, offsets, n, total_verts,
                           (const long long*)tile_start, (const MiBest*)partial, out);
    }
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

}  // extern "C"
