// On-device mesh rasteriser behind renderer.render: the reference renders every crop with PyBullet's
// OpenGL pipeline in a pool of worker processes (cosypose/rendering/bullet_batch_renderer.py:46-90,
// bullet_scene_renderer.py:38-60) and ships the images host -> device in EVERY iteration of the loop; this keeps the
// whole loop on the GPU.  Taken from the reference: the camera model (pixel i spans [i, i+1) in K coordinates, samples
// at i + 0.5: proj_from_K, simulator/camera.py:9-33), near plane 0.01, black background, float (B,3,H,W) in [0,1],
// non-finite poses -> black image (bullet_batch_renderer.py:25-36).  NOT reproducible: PyBullet's shading
// (third-party OpenGL renderer) -> pixel values are PARITY UNPINNED; the shading here is vertex colours x
// (ambient + diffuse |n.l|), flat per face.
//
// Pipeline per call, all crops at once (meshes of a few 10^3..10^4 triangles, a few pixels each at crop resolution):
//   1. project: one thread per (crop, vertex) -> (u, v, z_cam)
//   2. z-buffer: one thread per (crop, triangle) walks the triangle's pixel bounding box (raster_walk of raster_device.h: boxes
//      of more than 64 pixels are shared by the 64 lanes of the wave); edge functions at pixel centres; 64-bit atomicMin of
//      (depth bits << 32 | face id): order-independent, hence deterministic
//   3. resolve: one thread per pixel re-derives the barycentrics of the winning face, perspective-correct colour
//      interpolation, Lambert term from the camera-space face normal, clamps, writes planar RGB (+ depth).
// Near plane, where this differs from OpenGL: a triangle with ANY vertex at z <= 0.01 is dropped whole (the z-buffer pass tests the
// three vertices, not the pixel), where OpenGL clips it at the plane and keeps the part beyond.  An object that straddles the near
// plane loses its nearest triangles entirely; tests/test_raster_kernels.py exempts exactly those pixels from its float64 ray caster.
// The z-buffer pass puts the batch in gridDim.y: the wrappers refuse B > 65535 (COSY_MAX_GRID_Y) before any launch.
// fp32 with contraction off: oracle/cosy_oracle.c:cosy_oracle_rasterize is the same arithmetic in scalar loops and the
// GPU tests require identical face ids / depths.
#include "cosy_common.h"
#include "raster_device.h"

#pragma clang fp contract(off)

namespace cosy {
namespace {

__global__ __launch_bounds__(256) void raster_clear_kernel(unsigned long long* __restrict__ zbuf, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) zbuf[i] = ~0ull;
}

__global__ __launch_bounds__(256) void raster_project_kernel(const float* __restrict__ verts, const int* __restrict__ obj,
                                                             const float* __restrict__ TCO, const float* __restrict__ K, int V,
                                                             float* __restrict__ uvz) {
    const int b = blockIdx.y, v = blockIdx.x * 256 + threadIdx.x;
    if (v >= V) return;
    project_vertex(TCO + (size_t)b * 16, K + (size_t)b * 9, verts + ((size_t)obj[b] * V + v) * 3, uvz + ((size_t)b * V + v) * 3);
}

// one thread per (crop, triangle): the walk of raster_device.h, 64-bit atomicMin of (depth | face) into the crop's z-buffer
__global__ __launch_bounds__(256) void raster_tri_kernel(const float* __restrict__ uvz, const int* __restrict__ faces,
                                                         const int* __restrict__ n_faces, const int* __restrict__ obj,
                                                         const float* __restrict__ TCO, const float* __restrict__ K, int V, int F, int H,
                                                         int W, unsigned long long* __restrict__ zbuf) {
    const int b = blockIdx.y, f = blockIdx.x * 256 + threadIdx.x;
    const int o = obj[b];
    unsigned long long* zb = zbuf + (size_t)b * H * W;
    bool live = f < n_faces[o] && pose_finite(TCO + (size_t)b * 16, K + (size_t)b * 9);
    RasterTri t;
    if (live) live = raster_tri_setup(uvz + (size_t)b * V * 3, faces + ((size_t)o * F + f) * 3, H, W, t);
    raster_walk(live, t, f, [&](int tf, int x, int y, float z) {
        atomicMin(zb + (size_t)y * W + x, ((unsigned long long)__float_as_uint(z) << 32) | (unsigned int)tf);
    });
}

__global__ __launch_bounds__(256) void raster_resolve_kernel(const unsigned long long* __restrict__ zbuf, const float* __restrict__ uvz,
                                                             MeshView m, const int* __restrict__ obj, const float* __restrict__ TCO, int H,
                                                             int W, ShadeParams sp, float* __restrict__ rgb, float* __restrict__ depth) {
    const int b = blockIdx.y, pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= H * W) return;
    float out[3], zo;
    resolve_pixel(zbuf[(size_t)b * H * W + pix], uvz + (size_t)b * m.V * 3, m, obj[b], TCO + (size_t)b * 16, pix % W, pix / W, sp, out, zo);
#pragma unroll
    for (int k = 0; k < 3; ++k) rgb[((size_t)b * 3 + k) * H * W + pix] = out[k];
    if (depth) depth[(size_t)b * H * W + pix] = zo;
}

}  // namespace
}  // namespace cosy

using namespace cosy;

extern "C" {

size_t cosy_render_scratch_bytes(int B, int V, int H, int W) {
    // [z-buffer | projected vertices (padded to 32 bytes) | roi_align tap tables of the fused render + crop kernel]
    return (size_t)B * H * W * sizeof(unsigned long long) + (((size_t)B * V * 3 + 7) & ~(size_t)7) * sizeof(float) + crop_taps_bytes(B, H, W);
}

}  // extern "C"

namespace cosy {
// clear + project + z-buffer: fills `scratch` = [zbuf (B,H,W) u64 | uvz (B,V,3)]
int launch_render_zbuffer(const float* verts, const int* faces, const int* n_faces, const int* obj_id, const float* TCO, const float* K, int B,
                          int V, int F, int H, int W, void* scratch, hipStream_t s) {
    unsigned long long* zbuf = (unsigned long long*)scratch;
    float* uvz = (float*)(zbuf + (size_t)B * H * W);
    const long npx = (long)B * H * W;
    hipLaunchKernelGGL(raster_clear_kernel, dim3(cdiv(npx, 256)), dim3(256), 0, s, zbuf, npx);
    COSY_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(raster_project_kernel, dim3(cdiv(V, 256), B), dim3(256), 0, s, verts, obj_id, TCO, K, V, uvz);
    COSY_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(raster_tri_kernel, dim3(cdiv(F, 256), B), dim3(256), 0, s, (const float*)uvz, faces, n_faces, obj_id, TCO, K, V, F, H, W,
                       zbuf);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}
int check_mesh_shade(const cosy_mesh_t* mesh, const cosy_shade_t* shade, MeshView* m, ShadeParams* sp) {
    COSY_REQUIRE_PTR("render", mesh);
    COSY_REQUIRE_PTR("render", shade);
    COSY_REQUIRE(mesh->V > 0 && mesh->F > 0, "render: V=%d F=%d (both must be positive)", mesh->V, mesh->F);
    const float *verts = mesh->verts, *colors = mesh->colors;
    const int *faces = mesh->faces, *n_faces = mesh->n_faces;
    COSY_REQUIRE_PTR("render", verts);
    COSY_REQUIRE_PTR("render", colors);
    COSY_REQUIRE_PTR("render", faces);
    COSY_REQUIRE_PTR("render", n_faces);
    COSY_REQUIRE(!shade->smooth || mesh->normals, "render: smooth shading needs vertex normals (null normals)");
    COSY_REQUIRE(!mesh->tex || (mesh->uvs && mesh->TH > 0 && mesh->TW > 0), "render: a texture needs uvs and its size (uvs %s, TH=%d TW=%d)",
                 mesh->uvs ? "given" : "null", mesh->TH, mesh->TW);
    *m = MeshView{mesh->verts, mesh->colors, mesh->normals, mesh->uvs, mesh->tex, mesh->faces, mesh->V, mesh->F, mesh->TH, mesh->TW};
    *sp = ShadeParams{shade->ambient, shade->diffuse, shade->specular, shade->shininess, shade->light[0], shade->light[1], shade->light[2],
                      shade->light_frame, shade->smooth, shade->quantize};
    return COSY_OK;
}
int render_crop_pack(void* x, int dtype, const cosy_mesh_t* mesh, const cosy_shade_t* shade, const int* obj_id, const float* TCO,
                     const float* K_crop, const float* frames4, const int* im_id, const float* boxes, int B, int N, int h, int w, int H, int W,
                     void* scratch, hipStream_t s) {
    (void)N;
    MeshView m; ShadeParams sp;
    int rc;
    if ((rc = check_mesh_shade(mesh, shade, &m, &sp))) return rc;
    COSY_REQUIRE(B >= 0 && B <= COSY_MAX_GRID_Y, "render_crop_pack: B=%d outside [0, %d]", B, COSY_MAX_GRID_Y);   // B is gridDim.y of the z-buffer pass
    COSY_REQUIRE(H > 0 && W > 0 && h > 0 && w > 0, "render_crop_pack: bad sizes H=%d W=%d h=%d w=%d", H, W, h, w);
    COSY_REQUIRE(dtype == COSY_F32 || dtype == COSY_BF16 || dtype == COSY_F16, "render_crop_pack: dtype %d", dtype);
    if (B == 0) return COSY_OK;
    const void* x_nhwc8 = x;
    const float *frames_nhwc4 = frames4, *boxes_crop = boxes;
    COSY_REQUIRE_PTR("render_crop_pack", x_nhwc8);
    COSY_REQUIRE_PTR("render_crop_pack", obj_id);
    COSY_REQUIRE_PTR("render_crop_pack", TCO);
    COSY_REQUIRE_PTR("render_crop_pack", K_crop);
    COSY_REQUIRE_PTR("render_crop_pack", frames_nhwc4);
    COSY_REQUIRE_PTR("render_crop_pack", boxes_crop);
    COSY_REQUIRE_PTR("render_crop_pack", scratch);
    if ((rc = launch_render_zbuffer(m.verts, m.faces, mesh->n_faces, obj_id, TCO, K_crop, B, m.V, m.F, H, W, scratch, s))) return rc;
    return launch_render_crop_pack(x, dtype, frames4, im_id, boxes, scratch, m, obj_id, TCO, sp, B, h, w, H, W, s);
}
}  // namespace cosy

extern "C" {

int cosy_render_crop_pack_to(void* x_nhwc8, int dtype, const cosy_mesh_t* mesh, const cosy_shade_t* shade, const int* obj_id,
                             const float* TCO, const float* K_crop, const float* frames_nhwc4, const int* im_id, const float* boxes_crop,
                             int B, int N, int h, int w, int H, int W, void* scratch, cosy_stream_t stream) {
    return render_crop_pack(x_nhwc8, dtype, mesh, shade, obj_id, TCO, K_crop, frames_nhwc4, im_id, boxes_crop, B, N, h, w, H, W, scratch,
                            (hipStream_t)stream);
}

int cosy_render_meshes_ex(const cosy_mesh_t* mesh, const cosy_shade_t* shade, const int* obj_id, const float* TCO, const float* K, int B,
                          int H, int W, float* rgb, float* depth, void* scratch, cosy_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    MeshView m; ShadeParams sp;
    int rc;
    if ((rc = check_mesh_shade(mesh, shade, &m, &sp))) return rc;
    COSY_REQUIRE(B >= 0 && B <= COSY_MAX_GRID_Y, "render_meshes: B=%d outside [0, %d]", B, COSY_MAX_GRID_Y);   // B is gridDim.y of every pass
    COSY_REQUIRE(H > 0 && W > 0, "render_meshes: bad sizes H=%d W=%d", H, W);
    if (B == 0) return COSY_OK;
    COSY_REQUIRE_PTR("render_meshes", obj_id);
    COSY_REQUIRE_PTR("render_meshes", TCO);
    COSY_REQUIRE_PTR("render_meshes", K);
    COSY_REQUIRE_PTR("render_meshes", rgb);
    COSY_REQUIRE_PTR("render_meshes", scratch);
    if ((rc = launch_render_zbuffer(m.verts, m.faces, mesh->n_faces, obj_id, TCO, K, B, m.V, m.F, H, W, scratch, s))) return rc;
    const unsigned long long* zbuf = (const unsigned long long*)scratch;
    const float* uvz = (const float*)(zbuf + (size_t)B * H * W);
    hipLaunchKernelGGL(raster_resolve_kernel, dim3(cdiv(H * W, 256), B), dim3(256), 0, s, zbuf, uvz, m, obj_id, TCO, H, W, sp, rgb, depth);
    COSY_CHECK_HIP(hipGetLastError());
    return COSY_OK;
}

int cosy_render_meshes(const float* verts, const float* colors, const int* faces, const int* n_faces, const int* obj_id,
                       const float* TCO, const float* K, int B, int V, int F, int H, int W, float ambient, float diffuse,
                       float light_x, float light_y, float light_z, float* rgb, float* depth, void* scratch, cosy_stream_t stream) {
    cosy_mesh_t mesh{verts, colors, nullptr, nullptr, nullptr, faces, n_faces, V, F, 0, 0};
    cosy_shade_t shade{ambient, diffuse, 0.f, 1.f, {light_x, light_y, light_z}, 0, 0, 0};
    return cosy_render_meshes_ex(&mesh, &shade, obj_id, TCO, K, B, H, W, rgb, depth, scratch, stream);
}

}  // extern "C"
