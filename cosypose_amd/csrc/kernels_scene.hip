// Scene renderer: many object instances in many views, ONE shared z-buffer per view (interface of the reference's
// BulletSceneRenderer.render_scene, cosypose/rendering/bullet_scene_renderer.py:12-64; camera model, near plane and background
// handling as the batch rasteriser, kernels_raster.hip).  A ROW is one object instance in one view.  The route through the batch
// renderer costs one full-frame z-buffer, colour image and depth image per row and a depth composite afterwards; here a view's rows
// meet in the view's z-buffer and the per-row cost is the projected vertices and one bit per pixel.
//
// Passes of one call:
//   0. clear:   z-buffers to ~0, silhouette bits to 0, statistics to (0, empty box)
//   1. project: one thread per (row, vertex), the batch rasteriser's expression, K of the row's view
//   2. z-buffer: one thread per (row, triangle); liveness, pixel walk (raster_walk: boxes above 64 pixels shared by the wave) and
//      per-pixel arithmetic are the batch rasteriser's (raster_device.h).  64-bit atomicMin into the VIEW's z-buffer of
//          key = depth bits << 32 | slot << COSY_SCENE_FACE_BITS | face,
//      slot = the row's rank among the rows of its view in call order: the smaller depth wins, at equal depth bits the row that
//      comes first in the call, then the smaller face id.  An order-independent min: bit-reproducible.
//      The same walk records the row's SILHOUETTE -- the pixels any live triangle of the row covers, whatever is in front -- as
//      one bit per pixel per row (N x ceil(H W / 32) words, 32-bit atomicOr).  The one-thread walk gathers the bits of a word before
//      it touches memory, the wave-shared walk combines its lanes' bits with a ballot.
//   3. resolve: one thread per (view, pixel): slot -> row -> (object, TCO), the key re-packed as depth | face and handed to
//      resolve_pixel: shading is the batch renderer's bit for bit.  Background: the background colour, depth 0, mask -1.
//      Statistics of the winners (pixel count and box per row) with integer atomics, aggregated per wave first.
//   4. silhouette statistics: one thread per (row, word of its bit map): pixel count and box, aggregated per wave; then one
//      thread per row writes the counts and the float boxes.
// fp32 with contraction off, as the batch rasteriser: the tests require its CPU twin's face ids, depths and colours.
#include <vector>

#include "cosy_common.h"
#include "raster_device.h"
#include "reduce_device.h"

#pragma clang fp contract(off)

namespace cosy {
namespace {

constexpr int FACE_BITS = COSY_SCENE_FACE_BITS;
constexpr unsigned FACE_MASK = (1u << FACE_BITS) - 1u;
constexpr int SLOT_BITS = 32 - FACE_BITS;
constexpr int STAT = 10;        // per row: count_all, count_visib, box_obj (x0, y0, x1, y1), box_visib (x0, y0, x1, y1)
constexpr int EMPTY_MIN = 0x7fffffff, EMPTY_MAX = -1;

// scratch: [z-buffers (n_views,H,W) u64 | projected vertices (N,V,3) | id table | silhouette bits (N, words) | statistics (N,10)]
struct SceneLayout {
    size_t zbuf, uvz, table, sil, stat, total;
    int words;
};
// id table (int32): obj (N) | view (N) | slot (N) | view_off (n_views + 1) | view_rows (N): the rows of view v in call order are
// view_rows[view_off[v] .. view_off[v + 1])
size_t table_ints(int N, int n_views) { return 4 * (size_t)N + (size_t)n_views + 1; }
size_t pad32(size_t bytes) { return (bytes + 31) & ~(size_t)31; }
SceneLayout scene_layout(int N, int n_views, int V, int H, int W) {
    SceneLayout l;
    l.words = (int)(((size_t)H * W + 31) / 32);
    l.zbuf = 0;
    l.uvz = l.zbuf + (size_t)n_views * H * W * sizeof(unsigned long long);
    l.table = l.uvz + pad32((size_t)N * V * 3 * sizeof(float));
    l.sil = l.table + pad32(table_ints(N, n_views) * sizeof(int));
    l.stat = l.sil + pad32((size_t)N * l.words * sizeof(unsigned));
    l.total = l.stat + pad32((size_t)N * STAT * sizeof(int));
    return l;
}

__global__ __launch_bounds__(256) void scene_clear_kernel(unsigned long long* __restrict__ zbuf, long n_z, unsigned* __restrict__ sil, long n_sil,
                                                          int* __restrict__ stat, long n_stat) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n_z) zbuf[i] = ~0ull;
    if (i < n_sil) sil[i] = 0u;
    if (i < n_stat) {
        const int k = (int)(i % STAT);
        stat[i] = k < 2 ? 0 : ((k - 2) & 2) ? EMPTY_MAX : EMPTY_MIN;
    }
}

__global__ __launch_bounds__(256) void scene_project_kernel(const float* __restrict__ verts, const int* __restrict__ obj,
                                                            const int* __restrict__ view, const float* __restrict__ TCO,
                                                            const float* __restrict__ K, int V, float* __restrict__ uvz) {
    const int r = blockIdx.y, v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    project_vertex(TCO + (size_t)r * 16, K + (size_t)view[r] * 9, verts + ((size_t)obj[r] * V + v) * 3, uvz + ((size_t)r * V + v) * 3);
}

// The silhouette of a row as the hook of raster_walk: one bit per covered pixel into the row's bit map `sb` (null: none is
// recorded), without per-pixel atomics.
struct Silhouette {
    unsigned* sb;
    int W;
    int word = -1;
    unsigned bits = 0u;                              // own walk: covered pixels of the current word of the bit map
    __device__ __forceinline__ void thread_hit(int x, int y) {
        const int p = y * W + x;
        if ((p >> 5) != word) {
            thread_row_end();
            word = p >> 5;
        }
        bits |= 1u << (p & 31);
    }
    __device__ __forceinline__ void thread_row_end() {
        if (bits && sb) atomicOr(sb + word, bits);
        bits = 0u;
    }
    __device__ __forceinline__ void wave_step(bool in, bool hit, int x, int y, int xx, int bw) {
        const int lane = threadIdx.x & 63;
        const unsigned long long hits = __ballot(hit);
        if (sb && hits && in) {
            // Lanes lane, lane + 1, ... walk consecutive pixels of one box row: the first lane of each word of the bit map
            // (lane 0, the first pixel of a box row, or a pixel index that is a multiple of 32) writes the bits of all of them
            const int p = y * W + x;
            if (lane == 0 || xx == 0 || (p & 31) == 0) {
                const int run = min(min(bw - xx, 32 - (p & 31)), 64 - lane);
                const unsigned bits = ((unsigned)(hits >> lane) & (run >= 32 ? ~0u : (1u << run) - 1u)) << (p & 31);
                if (bits) atomicOr(sb + (p >> 5), bits);
            }
        }
    }
};

// one thread per (row, triangle): the walk of raster_device.h into the view's z-buffer, with the row's slot in the key and its
// silhouette.  sil == nullptr: no silhouette is recorded.
__global__ __launch_bounds__(256) void scene_tri_kernel(const float* __restrict__ uvz, const int* __restrict__ faces,
                                                        const int* __restrict__ n_faces, const int* __restrict__ obj,
                                                        const int* __restrict__ view, const int* __restrict__ slot,
                                                        const float* __restrict__ TCO, const float* __restrict__ K, int V, int F, int H, int W,
                                                        unsigned long long* __restrict__ zbuf, unsigned* __restrict__ sil, int words) {
    const int r = blockIdx.y, f = blockIdx.x * 256 + threadIdx.x;
    const int o = obj[r], vw = view[r];
    unsigned long long* zb = zbuf + (size_t)vw * H * W;
    const unsigned slot_bits = (unsigned)slot[r] << FACE_BITS;
    bool live = f < n_faces[o] && pose_finite(TCO + (size_t)r * 16, K + (size_t)vw * 9);
    RasterTri t;
    if (live) live = raster_tri_setup(uvz + (size_t)r * V * 3, faces + ((size_t)o * F + f) * 3, H, W, t);
    raster_walk(live, t, f, [&](int tf, int x, int y, float z) {
        atomicMin(zb + (size_t)y * W + x, ((unsigned long long)__float_as_uint(z) << 32) | slot_bits | (unsigned)tf);
    }, Silhouette{sil ? sil + (size_t)r * words : nullptr, W});
}

__device__ __forceinline__ void stat_box(int* box, int x0, int y0, int x1, int y1) {
    atomicMin(box, x0); atomicMin(box + 1, y0); atomicMax(box + 2, x1); atomicMax(box + 3, y1);
}

__global__ __launch_bounds__(256) void scene_resolve_kernel(const unsigned long long* __restrict__ zbuf, const float* __restrict__ uvz,
                                                            MeshView m, const int* __restrict__ obj, const int* __restrict__ view_off,
                                                            const int* __restrict__ view_rows, const float* __restrict__ TCO,
                                                            const float* __restrict__ color, int H, int W, ShadeParams sp, float bg0, float bg1,
                                                            float bg2, float* __restrict__ rgb, float* __restrict__ depth,
                                                            int* __restrict__ mask, int* __restrict__ stat) {
    const int vw = blockIdx.y, pix = blockIdx.x * 256 + threadIdx.x;
    const bool in = pix < H * W;
    int row = -1;
    const int x = pix % W, y = pix / W;
    if (in) {
        const unsigned long long key = zbuf[(size_t)vw * H * W + pix];
        float out[3] = {bg0, bg1, bg2}, zo = 0.f;
        if (key != ~0ull) {
            const unsigned low = (unsigned)(key & 0xffffffffu);
            row = view_rows[view_off[vw] + (int)(low >> FACE_BITS)];
            const float* ovr = (color && color[(size_t)row * 4 + 3] >= 0.f) ? color + (size_t)row * 4 : nullptr;
            resolve_pixel((key & 0xffffffff00000000ull) | (low & FACE_MASK), uvz + (size_t)row * m.V * 3, m, obj[row], TCO + (size_t)row * 16, x, y,
                          sp, out, zo, ovr);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) rgb[((size_t)vw * 3 + k) * H * W + pix] = out[k];
        if (depth) depth[(size_t)vw * H * W + pix] = zo;
        if (mask) mask[(size_t)vw * H * W + pix] = row;
    }
    if (!stat) return;
    // winners' statistics: one set of atomics per distinct row of the wave, not per pixel
    unsigned long long todo = __ballot(row >= 0);
    while (todo) {
        const int r = __builtin_amdgcn_readlane(row, __builtin_ctzll(todo));
        const bool mine = row == r;
        const unsigned long long who = __ballot(mine);
        todo &= ~who;
        const int x0 = wave_min(mine ? x : EMPTY_MIN), y0 = wave_min(mine ? y : EMPTY_MIN);
        const int x1 = wave_max(mine ? x : EMPTY_MAX), y1 = wave_max(mine ? y : EMPTY_MAX);
        if ((threadIdx.x & 63) == 0) {
            int* s = stat + (size_t)r * STAT;
            atomicAdd(s + 1, __builtin_popcountll(who));
            stat_box(s + 6, x0, y0, x1, y1);
        }
    }
}

__global__ __launch_bounds__(256) void scene_silhouette_stats_kernel(const unsigned* __restrict__ sil, int words, int W, int* __restrict__ stat) {
    const int r = blockIdx.y, w = blockIdx.x * 256 + threadIdx.x;
    unsigned bits = w < words ? sil[(size_t)r * words + w] : 0u;
    if (!__ballot(bits != 0u)) return;               // wave-uniform
    const int n = __builtin_popcount(bits);
    int x0 = EMPTY_MIN, y0 = EMPTY_MIN, x1 = EMPTY_MAX, y1 = EMPTY_MAX;
    while (bits) {                                   // a word may span several image rows when W is no multiple of 32
        const int p = w * 32 + __builtin_ctz(bits);
        bits &= bits - 1;
        const int y = p / W, x = p - y * W;
        x0 = min(x0, x); x1 = max(x1, x); y0 = min(y0, y); y1 = max(y1, y);
    }
    const int cnt = wave_sum(n);
    x0 = wave_min(x0); y0 = wave_min(y0); x1 = wave_max(x1); y1 = wave_max(y1);
    if ((threadIdx.x & 63) == 0) {
        int* s = stat + (size_t)r * STAT;
        atomicAdd(s, cnt);
        stat_box(s + 2, x0, y0, x1, y1);
    }
}

__global__ __launch_bounds__(256) void scene_stats_out_kernel(const int* __restrict__ stat, int N, int* __restrict__ px_count_all,
                                                              int* __restrict__ px_count_visib, float* __restrict__ bbox_obj,
                                                              float* __restrict__ bbox_visib) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= N) return;
    const int* s = stat + (size_t)r * STAT;
    px_count_all[r] = s[0];
    px_count_visib[r] = s[1];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        bbox_obj[r * 4 + k] = s[0] > 0 ? (float)s[2 + k] : -1.f;
        bbox_visib[r * 4 + k] = s[1] > 0 ? (float)s[6 + k] : -1.f;
    }
}

}  // namespace
}  // namespace cosy

using namespace cosy;

extern "C" {

size_t cosy_render_scene_scratch_bytes(int N, int n_views, int V, int H, int W) {
    if (N < 0 || n_views < 0 || V < 0 || H < 0 || W < 0) return 0;
    return scene_layout(N, n_views, V, H, W).total;
}

int cosy_render_scene(const cosy_mesh_t* mesh, const cosy_shade_t* shade, const int* host_obj_id, const int* host_view_id, const float* TCO,
                      const float* color, const float* K, int N, int n_views, int H, int W, const float* background, float* rgb, float* depth,
                      int* mask, int* px_count_all, int* px_count_visib, float* bbox_obj, float* bbox_visib, void* scratch,
                      cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    MeshView m; ShadeParams sp;
    int rc;
    if ((rc = check_mesh_shade(mesh, shade, &m, &sp))) return rc;
    COSY_REQUIRE(N >= 0 && N <= COSY_MAX_GRID_Y, "render_scene: N=%d outside [0, %d]", N, COSY_MAX_GRID_Y);   // rows are gridDim.y of passes 1, 2, 4
    COSY_REQUIRE(n_views >= 0 && n_views <= COSY_MAX_GRID_Y, "render_scene: n_views=%d outside [0, %d]", n_views, COSY_MAX_GRID_Y);   // ... of pass 3
    COSY_REQUIRE(H > 0 && W > 0, "render_scene: bad sizes H=%d W=%d", H, W);
    COSY_REQUIRE((long)H * W <= 0x7fffffffL - 64, "render_scene: H=%d W=%d: more pixels than an int32 index holds", H, W);
    COSY_REQUIRE(mesh->F <= COSY_SCENE_MAX_FACES, "render_scene: mesh->F=%d beyond the %d face bits of the z-buffer key (at most %d faces)", mesh->F,
                 COSY_SCENE_FACE_BITS, COSY_SCENE_MAX_FACES);
    const int n_stats = (px_count_all != nullptr) + (px_count_visib != nullptr) + (bbox_obj != nullptr) + (bbox_visib != nullptr);
    COSY_REQUIRE(n_stats == 0 || n_stats == 4, "render_scene: px_count_all, px_count_visib, bbox_obj and bbox_visib go together (%d of 4 given)", n_stats);
    if (n_views == 0 && N == 0) return COSY_OK;
    COSY_REQUIRE_PTR("render_scene", background);
    COSY_REQUIRE_PTR("render_scene", rgb);
    COSY_REQUIRE_PTR("render_scene", scratch);
    std::vector<int> table(table_ints(N, n_views), 0);
    int *t_obj = table.data(), *t_view = t_obj + N, *t_slot = t_view + N, *t_off = t_slot + N, *t_rows = t_off + n_views + 1;
    if (N > 0) {
        const int *obj_id = host_obj_id, *view_id = host_view_id;
        COSY_REQUIRE_PTR("render_scene", obj_id);
        COSY_REQUIRE_PTR("render_scene", view_id);
        COSY_REQUIRE_PTR("render_scene", TCO);
        COSY_REQUIRE_PTR("render_scene", K);
        for (int r = 0; r < N; ++r) {
            COSY_REQUIRE(view_id[r] >= 0 && view_id[r] < n_views, "render_scene: row %d: view_id %d outside [0, %d)", r, view_id[r], n_views);
            COSY_REQUIRE(obj_id[r] >= 0, "render_scene: row %d: obj_id %d is negative", r, obj_id[r]);
            t_off[view_id[r] + 1]++;
        }
        for (int v = 0; v < n_views; ++v) {
            COSY_REQUIRE(t_off[v + 1] <= COSY_SCENE_MAX_INSTANCES,
                         "render_scene: view %d holds %d instances, the z-buffer key admits %d per view (view_id)", v, t_off[v + 1],
                         COSY_SCENE_MAX_INSTANCES);
            t_off[v + 1] += t_off[v];
        }
        std::vector<int> fill(n_views, 0);
        for (int r = 0; r < N; ++r) {
            const int v = view_id[r];
            t_obj[r] = obj_id[r]; t_view[r] = v; t_slot[r] = fill[v];
            t_rows[t_off[v] + fill[v]++] = r;
        }
    }
    if (n_views == 0) return COSY_OK;                // rows checked, nothing to draw into

    const SceneLayout l = scene_layout(N, n_views, m.V, H, W);
    char* base = (char*)scratch;
    unsigned long long* zbuf = (unsigned long long*)(base + l.zbuf);
    float* uvz = (float*)(base + l.uvz);
    int* d_table = (int*)(base + l.table);
    const int *d_obj = d_table, *d_view = d_obj + N, *d_slot = d_view + N, *d_off = d_slot + N, *d_rows = d_off + n_views + 1;
    const bool stats = n_stats == 4 && N > 0;
    unsigned* sil = stats ? (unsigned*)(base + l.sil) : nullptr;
    int* stat = stats ? (int*)(base + l.stat) : nullptr;
    // pageable host memory: the runtime has consumed `table` when the call returns
    COSY_CHECK_HIP(hipMemcpyAsync(d_table, table.data(), table.size() * sizeof(int), hipMemcpyHostToDevice, s));
    const long n_z = (long)n_views * H * W, n_sil = stats ? (long)N * l.words : 0, n_stat = stats ? (long)N * STAT : 0;
    const long n_clear = n_z > n_sil ? (n_z > n_stat ? n_z : n_stat) : (n_sil > n_stat ? n_sil : n_stat);
    hipLaunchKernelGGL(scene_clear_kernel, dim3(cdiv(n_clear, 256)), dim3(256), 0, s, zbuf, n_z, sil, n_sil, stat, n_stat);
    COSY_CHECK_HIP(hipGetLastError());
    if (N > 0) {
        hipLaunchKernelGGL(scene_project_kernel, dim3(cdiv(m.V, 256), N), dim3(256), 0, s, m.verts, d_obj, d_view, TCO, K, m.V, uvz);
        COSY_CHECK_HIP(hipGetLastError());
        hipLaunchKernelGGL(scene_tri_kernel, dim3(cdiv(m.F, 256), N), dim3(256), 0, s, (const float*)uvz, m.faces, mesh->n_faces, d_obj, d_view, d_slot,
                           TCO, K, m.V, m.F, H, W, zbuf, sil, l.words);
        COSY_CHECK_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(scene_resolve_kernel, dim3(cdiv((long)H * W, 256), n_views), dim3(256), 0, s, (const unsigned long long*)zbuf,
                       (const float*)uvz, m, d_obj, d_off, d_rows, TCO, color, H, W, sp, background[0], background[1], background[2], rgb, depth,
                       mask, stat);
    COSY_CHECK_HIP(hipGetLastError());
    if (stats) {
        hipLaunchKernelGGL(scene_silhouette_stats_kernel, dim3(cdiv(l.words, 256), N), dim3(256), 0, s, (const unsigned*)sil, l.words, W, stat);
        COSY_CHECK_HIP(hipGetLastError());
        hipLaunchKernelGGL(scene_stats_out_kernel, dim3(cdiv(N, 256)), dim3(256), 0, s, (const int*)stat, N, px_count_all, px_count_visib, bbox_obj,
                           bbox_visib);
        COSY_CHECK_HIP(hipGetLastError());
    }
    return COSY_OK;
}

}  // extern "C"
