// BOP pose errors (Hodan et al., "BOP Challenge 2020", section 2.2): MSSD, MSPD and the pixel counts of VSD for B tentative
// (estimate, ground truth) pairs.  DESIGN.md section 15 holds the contract and the arithmetic; tests/bop_ref.py restates it in numpy.
//
// Step 1, MSSD + MSPD in one pass.  Work = a flat list of (pair, tile of BOP_TILE vertices, chunk of BOP_CH symmetries) items found
// from a prefix sum of the pairs' item counts (the queue of work_items.h): workgroups draw items from an integer counter, so
// the batch is no grid dimension and mixed mesh sizes keep the CUs busy.  Per item the chunk's ground-truth transforms P_gt S sit in
// LDS, every thread transforms its vertices once by P_est and keeps, per symmetry of the chunk, the running maximum of the squared
// 3-D and squared 2-D distance AS THE BIT PATTERN of a non-negative float.  Lanes, waves and tiles are combined by an integer max
// (shuffles, LDS atomics, global atomics on a zeroed table): order-independent, so two runs give equal bits and a pair alone gives
// what it gives inside a batch.  No floating-point atomics.  A last launch takes the square roots and the minimum over s < n_sym.
//
// Step 2, depth windows.  An instance is one (object, view, pose).  bop_box_kernel finds the pixel box of its live projected
// vertices clipped to the frame (integer min / max); the host sizes a packed store from the boxes; bop_zpass_kernel is the z-buffer
// pass of kernels_raster.hip -- raster_walk of raster_device.h at FULL-FRAME pixel coordinates, minimum of the depth bits --
// writing into the instance's window, so a window holds the bits the full-frame render has there.  The vertices are projected by the
// triangle's own thread with project_vertex of raster_device.h: no (N, V, 3) table of projected vertices exists.
//
// Step 3, VSD counts.  Work = a flat list of (pair, strip of VSD_STRIP pixels of the union box of the pair's two windows) items.
// Per pixel: the three distances from the three depths, the visibility masks, |U|, |I| and the n_tau cost counts by ballots and
// integer sums.
//
// Built with contraction off (build.py FILE_FLAGS): every product and sum is rounded on its own, as the numpy twins do.
#include <limits.h>
#include "cosy_common.h"
#include "bop_device.h"     // Window, window_of, window_index, window_depth, depth_to_dist, BOX_DEAD: shared with kernels_gt.hip
#include "raster_device.h"
#include "work_items.h"

#pragma clang fp contract(off)

namespace cosy {

namespace {

constexpr int BOP_G = 4;                     // vertices per thread
constexpr int BOP_TILE = 256 * BOP_G;        // vertices per work item
constexpr int BOP_CH = 8;                    // symmetries per work item
constexpr int BOP_GRID = 256 * 4;            // workgroups that draw items
constexpr int VSD_STRIP = 256 * 8;           // pixels per work item of step 3
constexpr int VSD_MAX_TAU = 16;

// ---- step 1 ---------------------------------------------------------------------------------------------------------------------
struct PairTables {
    const float* pred;      // (B,4,4)
    const float* gt;        // (B,4,4)
    const int* obj_id;      // (B)
    const int* view_id;     // (B)
    const float* K;         // (n_views,3,3)
    const float* verts;     // (n_obj,V,3)
    const int* n_verts;     // (n_obj)
    const float* sym;       // (n_obj,S,4,4)
    const int* n_sym;       // (n_obj)
    int B, n_obj, n_views, V, S;
};

// vertices and symmetries a pair works on; 0 / 0 where its ids lie outside the tables or a pose or K entry is not finite
__device__ __forceinline__ void pair_sizes(const PairTables& t, int b, int& nv, int& ns) {
    nv = ns = 0;
    const int o = t.obj_id[b], v = t.view_id[b];
    if (o < 0 || o >= t.n_obj || v < 0 || v >= t.n_views) return;
    if (!pose_finite(t.pred + (size_t)b * 16, t.K + (size_t)v * 9) || !pose_finite(t.gt + (size_t)b * 16, t.K + (size_t)v * 9)) return;
    nv = min(max(t.n_verts[o], 0), t.V);
    ns = min(max(t.n_sym[o], 0), t.S);
}

struct PairItems {
    PairTables t;
    __device__ int operator()(int b) const {
        int nv, ns;
        pair_sizes(t, b, nv, ns);
        return ((nv + BOP_TILE - 1) / BOP_TILE) * ((ns + BOP_CH - 1) / BOP_CH);
    }
};

__device__ __forceinline__ unsigned nonneg_bits(float v) { return __float_as_uint(v) & 0x7fffffffu; }     // a NaN stays a NaN and wins every max

__global__ __launch_bounds__(256) void bop_dist_kernel(PairTables t, WorkPlan* __restrict__ plan, const int* __restrict__ start,
                                                       unsigned* __restrict__ maxbits) {
    __shared__ float M[BOP_CH][12];          // rows 0..2 of P_gt S per symmetry of the chunk
    __shared__ unsigned red[2 * BOP_CH];
    const int tid = threadIdx.x;
    const int total = plan->total;
    for (;;) {
        const int item = next_item(plan);      // (a barrier: M and red of the previous item are no longer read)
        if (item >= total) return;
        const int b = row_of_item(start, t.B, item);
        int nv, ns;
        pair_sizes(t, b, nv, ns);              // nv, ns > 0 here: the pair has items
        const int n_chunks = (ns + BOP_CH - 1) / BOP_CH;
        const int local = item - start[b], tile = local / n_chunks, chunk = local - tile * n_chunks;
        const int nsc = min(BOP_CH, ns - chunk * BOP_CH);
        const int o = t.obj_id[b];
        const float* Kv = t.K + (size_t)t.view_id[b] * 9;
        const float fx = Kv[0], fy = Kv[4], cx = Kv[2], cy = Kv[5];
        const float* Tp = t.pred + (size_t)b * 16;
        const float* Tg = t.gt + (size_t)b * 16;
        if (tid < BOP_CH * 12) {
            const int s = tid / 12, e = tid - s * 12, i = e >> 2, j = e & 3;
            float v = 0.f;
            if (s < nsc) {
                const float* Sm = t.sym + ((size_t)o * t.S + chunk * BOP_CH + s) * 16;
                v = (Tg[i * 4] * Sm[j] + Tg[i * 4 + 1] * Sm[4 + j]) + Tg[i * 4 + 2] * Sm[8 + j];
                if (j == 3) v = v + Tg[i * 4 + 3];
            }
            M[s][e] = v;
        }
        if (tid < 2 * BOP_CH) red[tid] = 0u;
        __syncthreads();
        unsigned m3[BOP_CH], m2[BOP_CH];
#pragma unroll
        for (int s = 0; s < BOP_CH; ++s) m3[s] = m2[s] = 0u;
        const float* vb = t.verts + (size_t)o * t.V * 3;
#pragma unroll
        for (int k = 0; k < BOP_G; ++k) {
            const int vi = tile * BOP_TILE + k * 256 + tid;
            if (vi < nv) {
                const float x = vb[vi * 3], y = vb[vi * 3 + 1], z = vb[vi * 3 + 2];
                float q[3];
#pragma unroll
                for (int i = 0; i < 3; ++i) q[i] = ((Tp[i * 4] * x + Tp[i * 4 + 1] * y) + Tp[i * 4 + 2] * z) + Tp[i * 4 + 3];
                const float qu = fx * q[0] / q[2] + cx, qv = fy * q[1] / q[2] + cy;
#pragma unroll
                for (int s = 0; s < BOP_CH; ++s) {
                    if (s < nsc) {
                        float g[3];
#pragma unroll
                        for (int i = 0; i < 3; ++i) g[i] = ((M[s][i * 4] * x + M[s][i * 4 + 1] * y) + M[s][i * 4 + 2] * z) + M[s][i * 4 + 3];
                        const float dx = q[0] - g[0], dy = q[1] - g[1], dz = q[2] - g[2];
                        const float du = qu - (fx * g[0] / g[2] + cx), dv = qv - (fy * g[1] / g[2] + cy);
                        m3[s] = max(m3[s], nonneg_bits((dx * dx + dy * dy) + dz * dz));
                        m2[s] = max(m2[s], nonneg_bits(du * du + dv * dv));
                    }
                }
            }
        }
#pragma unroll
        for (int s = 0; s < BOP_CH; ++s) {
            m3[s] = wave_max(m3[s]); m2[s] = wave_max(m2[s]);
            if ((tid & 63) == 0 && s < nsc) { atomicMax(&red[2 * s], m3[s]); atomicMax(&red[2 * s + 1], m2[s]); }
        }
        __syncthreads();
        if (tid < 2 * nsc) atomicMax(maxbits + ((size_t)b * t.S + chunk * BOP_CH) * 2 + tid, red[tid]);
    }
}

// sqrt of the maxima and the minimum over the object's symmetries (a NaN entry is passed over unless every entry is one)
__global__ __launch_bounds__(256) void bop_dist_final_kernel(PairTables t, const unsigned* __restrict__ maxbits, float* __restrict__ mssd,
                                                             float* __restrict__ mspd) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= t.B) return;
    int nv, ns;
    pair_sizes(t, b, nv, ns);
    float e3 = __builtin_nanf(""), e2 = __builtin_nanf("");
    if (nv > 0)
        for (int s = 0; s < ns; ++s) {
            const float d3 = sqrtf(__uint_as_float(maxbits[((size_t)b * t.S + s) * 2]));
            const float d2 = sqrtf(__uint_as_float(maxbits[((size_t)b * t.S + s) * 2 + 1]));
            e3 = fminf(e3, d3);
            e2 = fminf(e2, d2);
        }
    mssd[b] = e3;
    mspd[b] = e2;
}

// ---- step 2 ---------------------------------------------------------------------------------------------------------------------
struct InstTables {
    const float* TCO;       // (N,4,4)
    const int* obj_id;      // (N)
    const int* view_id;     // (N)
    const float* K;         // (n_views,3,3)
    const float* verts;     // (n_obj,V,3)
    int N, n_obj, n_views, V;
};

__device__ __forceinline__ bool inst_live(const InstTables& t, int n) {
    const int o = t.obj_id[n], v = t.view_id[n];
    if (o < 0 || o >= t.n_obj || v < 0 || v >= t.n_views) return false;
    return pose_finite(t.TCO + (size_t)n * 16, t.K + (size_t)v * 9);
}

__global__ __launch_bounds__(256) void bop_box_init_kernel(InstTables t, int* __restrict__ boxes) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= t.N) return;
    const int hi = inst_live(t, n) ? -1 : BOX_DEAD;
    boxes[n * 4] = INT_MAX; boxes[n * 4 + 1] = INT_MAX; boxes[n * 4 + 2] = hi; boxes[n * 4 + 3] = hi;
}

// Box of the vertices beyond the near plane, each taken as raster_tri_setup takes a triangle's extreme vertex: floor(u - 0.5) clipped
// below at 0, ceil(u - 0.5) clipped above at W - 1.  A live triangle has all three vertices beyond the near plane, so its own pixel box
// lies inside this one.  The clipping happens in float (a NaN or huge coordinate widens the box to the frame's edge, never past it).
__global__ __launch_bounds__(256) void bop_box_kernel(InstTables t, const int* __restrict__ n_verts, int tiles, int H, int W,
                                                      int* __restrict__ boxes) {
    __shared__ int red[4];
    const int n = blockIdx.x / tiles, tile = blockIdx.x - n * tiles, tid = threadIdx.x;
    if (!inst_live(t, n)) return;            // block-uniform
    const int o = t.obj_id[n];
    const int nv = min(max(n_verts[o], 0), t.V);
    const int vi = tile * 256 + tid;
    if (tile * 256 >= nv) return;            // block-uniform
    int x0 = INT_MAX, y0 = INT_MAX, x1 = -1, y1 = -1;
    if (vi < nv) {
        float uvz[3];
        project_vertex(t.TCO + (size_t)n * 16, t.K + (size_t)t.view_id[n] * 9, t.verts + ((size_t)o * t.V + vi) * 3, uvz);
        if (uvz[2] > 0.01f) {
            x0 = (int)fminf(fmaxf(floorf(uvz[0] - 0.5f), 0.f), (float)W);
            y0 = (int)fminf(fmaxf(floorf(uvz[1] - 0.5f), 0.f), (float)H);
            x1 = (int)fmaxf(fminf(ceilf(uvz[0] - 0.5f), (float)(W - 1)), -1.f);
            y1 = (int)fmaxf(fminf(ceilf(uvz[1] - 0.5f), (float)(H - 1)), -1.f);
        }
    }
    if (tid < 4) red[tid] = tid < 2 ? INT_MAX : -1;
    __syncthreads();
    x0 = wave_min(x0); y0 = wave_min(y0); x1 = wave_max(x1); y1 = wave_max(y1);
    if ((tid & 63) == 0) { atomicMin(&red[0], x0); atomicMin(&red[1], y0); atomicMax(&red[2], x1); atomicMax(&red[3], y1); }
    __syncthreads();
    if (tid < 2) atomicMin(boxes + n * 4 + tid, red[tid]);
    else if (tid < 4) atomicMax(boxes + n * 4 + tid, red[tid]);
}

__global__ __launch_bounds__(256) void bop_fill_kernel(unsigned* __restrict__ p, long n, unsigned v) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = v;
}

// background (no triangle reached the pixel) -> depth 0, as the full-frame render writes it
__global__ __launch_bounds__(256) void bop_window_finish_kernel(unsigned* __restrict__ p, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n && p[i] == ~0u) p[i] = 0u;
}

// The z-buffer pass of the batch rasteriser (raster_walk of raster_device.h) on depth bits alone: one thread per (instance, triangle),
// the three vertices projected on the spot, 32-bit atomicMin into the instance's window.
__global__ __launch_bounds__(256) void bop_zpass_kernel(InstTables t, const int* __restrict__ faces, const int* __restrict__ n_faces, int F,
                                                        int tiles, int H, int W, const int* __restrict__ boxes,
                                                        const long long* __restrict__ win_offset, unsigned* __restrict__ store, long n_px) {
    const int n = blockIdx.x / tiles, tile = blockIdx.x - n * tiles;
    if (!inst_live(t, n)) return;            // block-uniform
    const Window w = window_of(boxes, win_offset, n_px, n, H, W);
    if (w.bw == 0) return;                   // block-uniform
    const int o = t.obj_id[n], f = tile * 256 + threadIdx.x;
    bool live = f < min(max(n_faces[o], 0), F);
    RasterTri tr;
    if (live) {
        const int* tri = faces + ((size_t)o * F + f) * 3;
        float uvz[9];
        const int idx[3] = {0, 1, 2};
        bool in_table = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int vi = tri[k];
            in_table = in_table && vi >= 0 && vi < t.V;
            if (in_table) project_vertex(t.TCO + (size_t)n * 16, t.K + (size_t)t.view_id[n] * 9, t.verts + ((size_t)o * t.V + vi) * 3, uvz + 3 * k);
        }
        live = in_table && raster_tri_setup(uvz, idx, H, W, tr);
    }
    raster_walk(live, tr, f, [&](int, int x, int y, float z) {
        const long at = window_index(w, x, y);
        if (at >= 0) atomicMin(store + at, __float_as_uint(z));
    });
}

// ---- step 3 ---------------------------------------------------------------------------------------------------------------------
struct VsdTables {
    const int* est_inst;            // (B) instance of the estimate
    const int* gt_inst;             // (B) instance of the ground truth
    const int* inst_view;           // (N)
    const int* boxes;               // (N,4)
    const long long* win_offset;    // (N)
    const float* store;             // the windows
    long n_px;
    const float* depth_test;        // (n_views,H,W)
    const float* K;                 // (n_views,3,3)
    int B, N, n_views, H, W;
};

struct VsdBox {
    int x0, y0, x1, y1;             // union of the two windows, empty: x1 < x0
    int view;
};

// the pair's two instances must lie in the table and in one view of the frame table; otherwise the pair has no pixels
__device__ __forceinline__ bool vsd_pair(const VsdTables& t, int b, Window& we, Window& wg, VsdBox& u) {
    u = VsdBox{0, 0, -1, -1, 0};
    const int e = t.est_inst[b], g = t.gt_inst[b];
    if (e < 0 || e >= t.N || g < 0 || g >= t.N) return false;
    const int v = t.inst_view[e];
    if (v < 0 || v >= t.n_views || t.inst_view[g] != v) return false;
    if (t.boxes[e * 4 + 2] == BOX_DEAD || t.boxes[g * 4 + 2] == BOX_DEAD) return false;
    we = window_of(t.boxes, t.win_offset, t.n_px, e, t.H, t.W);
    wg = window_of(t.boxes, t.win_offset, t.n_px, g, t.H, t.W);
    if (we.bw == 0 && wg.bw == 0) return false;
    u.view = v;
    if (we.bw == 0) { u.x0 = wg.x0; u.y0 = wg.y0; u.x1 = wg.x0 + wg.bw - 1; u.y1 = wg.y0 + wg.bh - 1; }
    else if (wg.bw == 0) { u.x0 = we.x0; u.y0 = we.y0; u.x1 = we.x0 + we.bw - 1; u.y1 = we.y0 + we.bh - 1; }
    else {
        u.x0 = min(we.x0, wg.x0); u.y0 = min(we.y0, wg.y0);
        u.x1 = max(we.x0 + we.bw, wg.x0 + wg.bw) - 1; u.y1 = max(we.y0 + we.bh, wg.y0 + wg.bh) - 1;
    }
    return true;
}

struct VsdItems {
    VsdTables t;
    __device__ int operator()(int b) const {
        Window we, wg;
        VsdBox u;
        if (!vsd_pair(t, b, we, wg, u)) return 0;
        const long px = (long)(u.x1 - u.x0 + 1) * (u.y1 - u.y0 + 1);
        return (int)((px + VSD_STRIP - 1) / VSD_STRIP);
    }
};

__global__ __launch_bounds__(256) void bop_vsd_kernel(VsdTables t, const float* __restrict__ taus, int n_tau, float delta, WorkPlan* __restrict__ plan,
                                                      const int* __restrict__ start, int* __restrict__ counts) {
    __shared__ int red[4][2 + VSD_MAX_TAU];
    const int tid = threadIdx.x, wave = tid >> 6;
    const int total = plan->total;
    for (;;) {
        const int item = next_item(plan);
        if (item >= total) return;
        const int b = row_of_item(start, t.B, item);
        Window we, wg;
        VsdBox u;
        if (!vsd_pair(t, b, we, wg, u)) continue;       // (a pair with items has pixels; block-uniform)
        const int strip = item - start[b];
        const int bw = u.x1 - u.x0 + 1;
        const long npx = (long)bw * (u.y1 - u.y0 + 1);
        const float* Kv = t.K + (size_t)u.view * 9;
        const float fx = Kv[0], fy = Kv[4], cx = Kv[2], cy = Kv[5];
        const float* frame = t.depth_test + (size_t)u.view * t.H * t.W;
        float tau[VSD_MAX_TAU];
#pragma unroll
        for (int k = 0; k < VSD_MAX_TAU; ++k) tau[k] = k < n_tau ? taus[(size_t)b * n_tau + k] : 0.f;
        int n_u = 0, n_i = 0, c[VSD_MAX_TAU];
#pragma unroll
        for (int k = 0; k < VSD_MAX_TAU; ++k) c[k] = 0;
        for (int j = 0; j < VSD_STRIP / 256; ++j) {
            const long i = (long)strip * VSD_STRIP + j * 256 + tid;
            bool in_u = false, in_i = false;
            float diff = 0.f;
            if (i < npx) {
                const int yy = (int)(i / bw), x = u.x0 + (int)(i - (long)yy * bw), y = u.y0 + yy;      // inside the frame: window_of admits no other box
                const float xc = (float)x - cx, yc = (float)y - cy;
                const float de = depth_to_dist(window_depth(we, t.store, x, y), xc, yc, fx, fy);
                const float dg = depth_to_dist(window_depth(wg, t.store, x, y), xc, yc, fx, fy);
                const float dt = depth_to_dist(frame[(size_t)y * t.W + x], xc, yc, fx, fy);
                const bool v_gt = dg > 0.f && (dg - dt <= delta || dt == 0.f);
                const bool v_est = (de > 0.f && (de - dt <= delta || dt == 0.f)) || (v_gt && de > 0.f);
                in_u = v_gt || v_est;
                in_i = v_gt && v_est;
                diff = fabsf(dg - de);
            }
            n_u += __popcll(__ballot(in_u));
            n_i += __popcll(__ballot(in_i));
#pragma unroll
            for (int k = 0; k < VSD_MAX_TAU; ++k) c[k] += __popcll(__ballot(k < n_tau && in_i && diff >= tau[k]));
        }
        if ((tid & 63) == 0) {
            red[wave][0] = n_u; red[wave][1] = n_i;
#pragma unroll
            for (int k = 0; k < VSD_MAX_TAU; ++k) red[wave][2 + k] = c[k];
        }
        __syncthreads();
        if (tid < 2 + n_tau) {
            const int sum = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
            if (sum) atomicAdd(counts + (size_t)b * (2 + n_tau) + tid, sum);
        }
    }
}

}  // namespace

}  // namespace cosy

using namespace cosy;

extern "C" {

size_t cosy_bop_mssd_mspd_workspace_bytes(int B, int S) {
    if (B <= 0 || S <= 0) return 0;
    return work_plan_bytes(B) + (size_t)B * S * 2 * sizeof(unsigned);
}

int cosy_bop_mssd_mspd(const float* TCO_pred, const float* TCO_gt, const int* obj_id, const int* view_id, const float* K, const float* verts,
                       const int* n_verts, const float* sym_table, const int* n_sym, int B, int n_obj, int n_views, int V, int S, float* mssd,
                       float* mspd, void* workspace, size_t workspace_bytes, cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    COSY_REQUIRE(B >= 0 && n_obj > 0 && n_views > 0 && V > 0 && S > 0, "cosy_bop_mssd_mspd: B=%d n_obj=%d n_views=%d V=%d S=%d", B, n_obj, n_views, V,
                 S);
    const long per_pair = (long)cdiv(V, BOP_TILE) * cdiv(S, BOP_CH);
    COSY_REQUIRE((long)B * per_pair < (1L << 31), "cosy_bop_mssd_mspd: B=%d x %ld items of V=%d S=%d exceed 2^31 items", B, per_pair, V, S);
    if (B == 0) return COSY_OK;
    COSY_REQUIRE_PTR("cosy_bop_mssd_mspd", TCO_pred); COSY_REQUIRE_PTR("cosy_bop_mssd_mspd", TCO_gt);
    COSY_REQUIRE_PTR("cosy_bop_mssd_mspd", obj_id); COSY_REQUIRE_PTR("cosy_bop_mssd_mspd", view_id);
    COSY_REQUIRE_PTR("cosy_bop_mssd_mspd", K); COSY_REQUIRE_PTR("cosy_bop_mssd_mspd", verts);
    COSY_REQUIRE_PTR("cosy_bop_mssd_mspd", n_verts); COSY_REQUIRE_PTR("cosy_bop_mssd_mspd", sym_table);
    COSY_REQUIRE_PTR("cosy_bop_mssd_mspd", n_sym); COSY_REQUIRE_PTR("cosy_bop_mssd_mspd", mssd);
    COSY_REQUIRE_PTR("cosy_bop_mssd_mspd", mspd); COSY_REQUIRE_PTR("cosy_bop_mssd_mspd", workspace);
    COSY_REQUIRE(workspace_bytes >= cosy_bop_mssd_mspd_workspace_bytes(B, S), "cosy_bop_mssd_mspd: workspace_bytes=%zu < %zu", workspace_bytes,
                 cosy_bop_mssd_mspd_workspace_bytes(B, S));
    COSY_REQUIRE(((uintptr_t)workspace & 15) == 0, "cosy_bop_mssd_mspd: workspace not 16-byte aligned");
    WorkPlan* plan = (WorkPlan*)workspace;
    int* start = (int*)(plan + 1);
    unsigned* maxbits = (unsigned*)((char*)workspace + work_plan_bytes(B));
    const PairTables t{TCO_pred, TCO_gt, obj_id, view_id, K, verts, n_verts, sym_table, n_sym, B, n_obj, n_views, V, S};
    COSY_CHECK_HIP(hipMemsetAsync(maxbits, 0, (size_t)B * S * 2 * sizeof(unsigned), s));
    hipLaunchKernelGGL(work_plan_kernel<PairItems>, dim3(1), dim3(256), 0, s, PairItems{t}, B, plan, start);
    COSY_CHECK_HIP(hipGetLastError());
    const long max_items = (long)B * per_pair;
    hipLaunchKernelGGL(bop_dist_kernel, dim3((unsigned)(max_items < BOP_GRID ? max_items : BOP_GRID)), dim3(256), 0, s, t, plan, (const int*)start,
                       maxbits);
    COSY_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(bop_dist_final_kernel, dim3(cdiv(B, 256)), dim3(256), 0, s, t, (const unsigned*)maxbits, mssd, mspd);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

int cosy_bop_instance_boxes(const float* TCO, const int* obj_id, const int* view_id, const float* K, const float* verts, const int* n_verts,
                            int N, int n_obj, int n_views, int V, int H, int W, int* boxes, cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    COSY_REQUIRE(N >= 0 && n_obj > 0 && n_views > 0 && V > 0 && H > 0 && W > 0, "cosy_bop_instance_boxes: N=%d n_obj=%d n_views=%d V=%d H=%d W=%d", N,
                 n_obj, n_views, V, H, W);
    COSY_REQUIRE((long)N * cdiv(V, 256) < (1L << 31), "cosy_bop_instance_boxes: N=%d x %d blocks of V=%d exceed 2^31", N, cdiv(V, 256), V);
    if (N == 0) return COSY_OK;
    COSY_REQUIRE_PTR("cosy_bop_instance_boxes", TCO); COSY_REQUIRE_PTR("cosy_bop_instance_boxes", obj_id);
    COSY_REQUIRE_PTR("cosy_bop_instance_boxes", view_id); COSY_REQUIRE_PTR("cosy_bop_instance_boxes", K);
    COSY_REQUIRE_PTR("cosy_bop_instance_boxes", verts); COSY_REQUIRE_PTR("cosy_bop_instance_boxes", n_verts);
    COSY_REQUIRE_PTR("cosy_bop_instance_boxes", boxes);
    const InstTables t{TCO, obj_id, view_id, K, verts, N, n_obj, n_views, V};
    hipLaunchKernelGGL(bop_box_init_kernel, dim3(cdiv(N, 256)), dim3(256), 0, s, t, boxes);
    COSY_CHECK_HIP(hipGetLastError());
    const int tiles = cdiv(V, 256);
    hipLaunchKernelGGL(bop_box_kernel, dim3((unsigned)((long)N * tiles)), dim3(256), 0, s, t, n_verts, tiles, H, W, boxes);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

size_t cosy_bop_windows_workspace_bytes(long long n_pixels) { return n_pixels <= 0 ? 0 : ((size_t)n_pixels * sizeof(float) + 15) / 16 * 16; }

int cosy_bop_render_windows(const float* TCO, const int* obj_id, const int* view_id, const float* K, const float* verts, const int* faces,
                            const int* n_faces, const int* boxes, const long long* win_offset, int N, int n_obj, int n_views, int V, int F, int H,
                            int W, long long n_pixels, void* workspace, size_t workspace_bytes, cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    COSY_REQUIRE(N >= 0 && n_obj > 0 && n_views > 0 && V > 0 && F > 0 && H > 0 && W > 0 && n_pixels >= 0,
                 "cosy_bop_render_windows: N=%d n_obj=%d n_views=%d V=%d F=%d H=%d W=%d n_pixels=%lld", N, n_obj, n_views, V, F, H, W, n_pixels);
    COSY_REQUIRE((long)N * cdiv(F, 256) < (1L << 31), "cosy_bop_render_windows: N=%d x %d blocks of F=%d exceed 2^31", N, cdiv(F, 256), F);
    if (N == 0 || n_pixels == 0) return COSY_OK;
    COSY_REQUIRE_PTR("cosy_bop_render_windows", TCO); COSY_REQUIRE_PTR("cosy_bop_render_windows", obj_id);
    COSY_REQUIRE_PTR("cosy_bop_render_windows", view_id); COSY_REQUIRE_PTR("cosy_bop_render_windows", K);
    COSY_REQUIRE_PTR("cosy_bop_render_windows", verts); COSY_REQUIRE_PTR("cosy_bop_render_windows", faces);
    COSY_REQUIRE_PTR("cosy_bop_render_windows", n_faces); COSY_REQUIRE_PTR("cosy_bop_render_windows", boxes);
    COSY_REQUIRE_PTR("cosy_bop_render_windows", win_offset); COSY_REQUIRE_PTR("cosy_bop_render_windows", workspace);
    COSY_REQUIRE(workspace_bytes >= cosy_bop_windows_workspace_bytes(n_pixels), "cosy_bop_render_windows: workspace_bytes=%zu < %zu", workspace_bytes,
                 cosy_bop_windows_workspace_bytes(n_pixels));
    COSY_REQUIRE(((uintptr_t)workspace & 15) == 0, "cosy_bop_render_windows: workspace not 16-byte aligned");
    const InstTables t{TCO, obj_id, view_id, K, verts, N, n_obj, n_views, V};
    unsigned* store = (unsigned*)workspace;
    hipLaunchKernelGGL(bop_fill_kernel, dim3(cdiv(n_pixels, 256)), dim3(256), 0, s, store, (long)n_pixels, ~0u);
    COSY_CHECK_HIP(hipGetLastError());
    const int tiles = cdiv(F, 256);
    hipLaunchKernelGGL(bop_zpass_kernel, dim3((unsigned)((long)N * tiles)), dim3(256), 0, s, t, faces, n_faces, F, tiles, H, W, boxes, win_offset, store,
                       (long)n_pixels);
    COSY_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(bop_window_finish_kernel, dim3(cdiv(n_pixels, 256)), dim3(256), 0, s, store, (long)n_pixels);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

size_t cosy_bop_vsd_workspace_bytes(int B) { return B <= 0 ? 0 : work_plan_bytes(B); }

int cosy_bop_vsd_counts(const int* est_inst, const int* gt_inst, const int* inst_view, const int* boxes, const long long* win_offset,
                        const float* windows, long long n_pixels, const float* depth_test, const float* K, const float* taus, float delta, int B,
                        int N, int n_views, int n_tau, int H, int W, int* counts, void* workspace, size_t workspace_bytes,
                        cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    COSY_REQUIRE(B >= 0 && N >= 0 && n_views > 0 && H > 0 && W > 0 && n_pixels >= 0, "cosy_bop_vsd_counts: B=%d N=%d n_views=%d H=%d W=%d n_pixels=%lld",
                 B, N, n_views, H, W, n_pixels);
    COSY_REQUIRE(n_tau >= 1 && n_tau <= VSD_MAX_TAU, "cosy_bop_vsd_counts: n_tau=%d outside [1, %d]", n_tau, VSD_MAX_TAU);
    COSY_REQUIRE((long)B * cdiv((long)H * W, VSD_STRIP) < (1L << 31), "cosy_bop_vsd_counts: B=%d x %d strips of H=%d W=%d exceed 2^31 items", B,
                 cdiv((long)H * W, VSD_STRIP), H, W);
    if (B == 0) return COSY_OK;
    COSY_REQUIRE_PTR("cosy_bop_vsd_counts", est_inst); COSY_REQUIRE_PTR("cosy_bop_vsd_counts", gt_inst);
    COSY_REQUIRE_PTR("cosy_bop_vsd_counts", depth_test); COSY_REQUIRE_PTR("cosy_bop_vsd_counts", K);
    COSY_REQUIRE_PTR("cosy_bop_vsd_counts", taus); COSY_REQUIRE_PTR("cosy_bop_vsd_counts", counts);
    COSY_REQUIRE_PTR("cosy_bop_vsd_counts", workspace);
    COSY_REQUIRE(N == 0 || (inst_view && boxes && win_offset), "cosy_bop_vsd_counts: null inst_view, boxes or win_offset with N=%d", N);
    COSY_REQUIRE(n_pixels == 0 || windows, "cosy_bop_vsd_counts: null windows with n_pixels=%lld", n_pixels);
    COSY_REQUIRE(workspace_bytes >= cosy_bop_vsd_workspace_bytes(B), "cosy_bop_vsd_counts: workspace_bytes=%zu < %zu", workspace_bytes,
                 cosy_bop_vsd_workspace_bytes(B));
    COSY_REQUIRE(((uintptr_t)workspace & 15) == 0, "cosy_bop_vsd_counts: workspace not 16-byte aligned");
    WorkPlan* plan = (WorkPlan*)workspace;
    int* start = (int*)(plan + 1);
    const VsdTables t{est_inst, gt_inst, inst_view, boxes, win_offset, windows, (long)n_pixels, depth_test, K, B, N, n_views, H, W};
    COSY_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)B * (2 + n_tau) * sizeof(int), s));
    hipLaunchKernelGGL(work_plan_kernel<VsdItems>, dim3(1), dim3(256), 0, s, VsdItems{t}, B, plan, start);
    COSY_CHECK_HIP(hipGetLastError());
    const long max_items = (long)B * cdiv((long)H * W, VSD_STRIP);
    hipLaunchKernelGGL(bop_vsd_kernel, dim3((unsigned)(max_items < BOP_GRID ? max_items : BOP_GRID)), dim3(256), 0, s, t, taus, n_tau, delta, plan,
                       (const int*)start, counts);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

}  // extern "C"
