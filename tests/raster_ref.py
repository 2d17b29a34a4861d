"""Float64 ray caster and shader: the independent reference of the mesh rasteriser, and the case matrix of
tests/test_raster_kernels.py.  A helper module (like ransac_case.py / train_case.py), numpy only on the reference side.

The rasteriser (csrc/kernels_raster.hip, raster_device.h) and its CPU twin (oracle/cosy_oracle.c) work in the image plane:
project the vertices, evaluate 2-D edge functions at pixel centres, interpolate w/z.  This module shares none of that.  It
shoots the camera ray of a pixel through the 3-D triangles (Moeller-Trumbore) and shades from the 3-D barycentrics of the hit:

  ray of sample (px, py) = (x + 0.5 + ox, y + 0.5 + oy):   d = ((px - cx) / fx, (py - cy) / fy, 1), origin 0
  triangle (A, B, C) = float32 inputs promoted to float64, moved by TCO;  e1 = B - A, e2 = C - A
  p = d x e2, det = e1 . p, u = (-A . p) / det, q = -A x e1, v = (d . q) / det, t = (e2 . q) / det
  hit: u >= 0, v >= 0, u + v <= 1; depth = t (d_z = 1); the nearest hit with depth > 0.01 wins (OpenGL's near clipping, per pixel);
  equal depths: the lower face id.  Barycentrics of the hit: (1 - u - v, u, v).

Five samples per pixel, offsets (0,0), (+-D,0), (0,+-D) with D = 2^-10 px, decide what can be compared at all:

  depth-comparable : all five hit or all five miss, and the five depths span <= 1e-4 relative.  Silhouettes and occlusion
                     boundaries drop out; an interior shared edge does NOT (both faces give the same surface), so a crack shows.
  colour-comparable: flat shading: all five hit the same face;  smooth shading: depth-comparable.
  near-exempt      : the winning triangle of the reference (centre sample) or of the rasteriser has a vertex at z <= 0.01.
                     Reason: "whole-triangle near rule, where OpenGL clips" -- the rasteriser drops such a triangle whole.

DEPTH BOUND.  |z - z_ref| <= z_ref * EPS32 * (C0 + KAPPA * cond),  cond = S L / |A| * dz / z_min, all from the float64
reference triangle: S the largest absolute projected coordinate of its vertices (before or after adding the principal point --
both are rounded), L its longest projected edge, A its projected parallelogram area (the value of the edge function at the third
vertex, = 2 x the triangle's area: what the rasteriser divides by), dz its depth range, z_min its nearest vertex.  EPS32 = 2^-23;
one float32 rounding is at most EPS32 / 2 relative.  Counted, not fitted:

  KAPPA.  A stored projected coordinate u = fl(fl(fl(fx X) / Z) + cx) has gone through 15 roundings, each at most
  (EPS32/2) S in pixels: X = ((T0 p0 + T1 p1) + T2 p2) + T3 is 3 products + 3 sums (6), the same for Z (6; its relative error
  moves u by at most |u - cx| <= S), then the product, the quotient and the sum (3).  Both coordinates of a vertex are off by
  that much, so the vertex is displaced by d with |d| <= sqrt(2) * 15 * (EPS32/2) * S.  Displacing vertex j by d_j changes any
  attribute q that is linear over the triangle by -sum_j w_j d_j . grad q at the pixel, and sum_j w_j = 1 with w_j >= 0 inside, so
  |delta q| <= max |d_j| |grad q|.  For q = 1/z: |grad q| <= range(1/z) / (least width of the triangle) = dz / (z_min z_max) * L / |A|.
  Hence |delta z| / z = z |delta (1/z)| <= sqrt(2) * 7.5 * EPS32 * S L / |A| * dz / z_min:  KAPPA = 7.5 sqrt(2) = 10.6.

  C0.  What remains when dz = 0, roundings relative to z itself.  An edge function E = P1 - P2 with P = fl(fl(difference) *
  fl(difference)) carries 3 roundings per product and one for the subtraction: |delta E| <= (EPS32/2) (3 |P1| + 3 |P2| + |E|), which is
  4 roundings of E where the products do not cancel (|P1| + |P2| = |E|).  The pixel's three edge functions enter z as a convex
  combination (4, counted once), the area's own edge function (4), 1 / area (1), E_i * (1 / area) (1), w_i / z_i (1), the two
  sums (2), the final reciprocal (1), and Z of the vertices, 3 products + 3 sums (6, a convex combination again): 20 roundings of
  at most EPS32/2:  C0 = 10.
  (Where the two products of an edge function DO cancel -- a needle that is not axis-aligned -- their roundings exceed |E| by up
  to L^2 / |A| <= 2 S L / |A|, a term that is not multiplied by dz / z_min.  It is the one thing this bound neglects; the needle
  case has dz / z_min of a few per cent and stays inside the bound.)

  Measured worst |z - z_ref| / bound, twin and kernel alike (the kernel is bit-equal to the twin): 0.80 on the needle fan, 0.77 at
  f = 2600, 0.16 - 0.40 elsewhere; the median bound of the usual poses is 1.9e-6 relative (asserted below 2e-6: the bound is not vacuous).

COLOUR BOUND.  The same displacement argument with q = the colour: |delta c| <= max |d_j| |grad c|, and
|grad c| <= (colour range over the triangle) * L / |A|.  The colour range is taken from the reference: the largest of the range of the
reference colour at the triangle's three vertices and the finite-difference gradient of the five samples times the triangle's least
width |A| / L (a texture or a highlight varies inside a triangle).  Bound: EPS32 * KAPPA * S L / |A| * range + FLOOR.  FLOOR is
3 x the worst deviation of this module's own shading formula evaluated in float32 numpy at the float64 hit points from its
float64 evaluation -- the reference rounded, not the kernel -- over the case's colour-comparable pixels:
the table FLOOR_MEASURED below, one figure per case (1.5e-7 for smooth shading at arm's length up to 1.9e-4 for the flat normal of
a needle).  With quantize = 1 the output is k/255: at most one step of difference, only on values whose unrounded reference lies
within the bound of a rounding threshold, and on no more values than the float32 evaluation itself flips.

CPU cost, measured: the references of the whole matrix take about 20 s on one core (usual_240x320 3.2 s and b17 4.9 s are the
long ones, a 96x128 case 0.2 - 1 s); each case is cast once per process (Case.reference is cached) and shared by all tests.
"""
import functools

import numpy as np

EPS32 = float(np.finfo(np.float32).eps)        # 2^-23
C0, KAPPA = 10.0, 7.5 * 2 ** 0.5                # counted in the docstring above
NEAR = 0.01
DELTA = 2.0 ** -10
OFFSETS = ((0.0, 0.0), (DELTA, 0.0), (-DELTA, 0.0), (0.0, DELTA), (0.0, -DELTA))
DEPTH_SPAN = 1e-4
# Colour floor per case = 3 x FLOOR_MEASURED: the worst |float32 evaluation - float64 evaluation| of shade() below at the float64 hit
# points over the case's colour-comparable pixels (float32_floor(); test_colour_floor_is_the_float32_reference re-measures it).  The
# flat-shaded cases are the large ones: the face normal is a cross product of float32 edge vectors of millimetre triangles seen at
# metres (far, b17), or of needles -- the rounded reference itself is that uncertain there.
FLOOR_MEASURED = {
    'usual_240x320': 4.57e-06, 'b1': 1.59e-07, 'b17': 2.49e-05, 'size_45x61': 5.50e-07, 'size_48x64': 4.97e-07, 'far': 2.29e-05,
    'close_offscreen': 6.05e-07, 'offscreen': 0.0, 'near_plane': 6.47e-07, 'pp_outside': 1.61e-07, 'f2600': 5.31e-07,
    'coarse_mixed': 7.13e-06, 'interpenetrating': 1.93e-07, 'needle_fan': 1.92e-04, 'padded_mixed_VF': 1.53e-07, 'mirror': 3.91e-07,
    'exact_tie': 0.0,
}
FLOOR = {k: 3 * v for k, v in FLOOR_MEASURED.items()}
NEAR_REASON = 'whole-triangle near rule, where OpenGL clips'


# ---------------------------------------------------------------------------------------------------------------------
# geometry: nearest ray hit per sample
# ---------------------------------------------------------------------------------------------------------------------
def cast(P, faces, K, H, W, offsets=OFFSETS):
    """P (V,3) float64 camera-frame vertices, faces (F,3), K (3,3) -> depth (S,H,W) (inf = miss), face (S,H,W) (-1 = miss),
    bary (S,H,W,3).  Per-triangle loop over the pixel box of the triangle's projection (the whole image when the triangle
    reaches behind the camera)."""
    S = len(offsets)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    depth = np.full((S, H, W), np.inf); face = np.full((S, H, W), -1, np.int64); bary = np.zeros((S, H, W, 3))
    off = np.asarray(offsets, np.float64)
    for f, (ia, ib, ic) in enumerate(np.asarray(faces)):
        A, B, C = P[ia], P[ib], P[ic]
        zs = np.array([A[2], B[2], C[2]])
        if zs.max() <= NEAR:
            continue                                      # no part of it beyond the near plane
        if zs.min() > 1e-6:
            us = fx * np.array([A[0], B[0], C[0]]) / zs + cx; vs = fy * np.array([A[1], B[1], C[1]]) / zs + cy
            x0, x1 = int(np.floor(us.min() - 1.5)), int(np.ceil(us.max() + 0.5))
            y0, y1 = int(np.floor(vs.min() - 1.5)), int(np.ceil(vs.max() + 0.5))
            x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, W - 1), min(y1, H - 1)
            if x1 < x0 or y1 < y0:
                continue
        else:
            x0, y0, x1, y1 = 0, 0, W - 1, H - 1
        e1, e2 = B - A, C - A
        px = np.arange(x0, x1 + 1) + 0.5; py = np.arange(y0, y1 + 1) + 0.5
        dx = (px[None, None, :] + off[:, 0, None, None] - cx) / fx                       # (S,1,w)
        dy = (py[None, :, None] + off[:, 1, None, None] - cy) / fy                       # (S,h,1)
        # p = d x e2 with d = (dx, dy, 1)
        p0 = dy * e2[2] - e2[1]; p1 = e2[0] - dx * e2[2]; p2 = dx * e2[1] - dy * e2[0]
        det = e1[0] * p0 + e1[1] * p1 + e1[2] * p2
        with np.errstate(divide='ignore', invalid='ignore'):
            u = -(A[0] * p0 + A[1] * p1 + A[2] * p2) / det
            q = -np.cross(A, e1)
            v = (dx * q[0] + dy * q[1] + q[2]) / det
            t = (e2 @ q) / det
        hit = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > NEAR)
        sub_d = depth[:, y0:y1 + 1, x0:x1 + 1]
        hit &= t < sub_d                                   # strict: at equal depth the lower face id stays
        if not hit.any():
            continue
        sub_d[hit] = np.broadcast_to(t, hit.shape)[hit]
        face[:, y0:y1 + 1, x0:x1 + 1][hit] = f
        sb = bary[:, y0:y1 + 1, x0:x1 + 1]
        uu, vv = np.broadcast_to(u, hit.shape)[hit], np.broadcast_to(v, hit.shape)[hit]
        sb[hit] = np.stack([1 - uu - vv, uu, vv], -1)
    return depth, face, bary


# ---------------------------------------------------------------------------------------------------------------------
# shading from 3-D barycentrics (include/cosyhip.h: cosy_shade_t, cosy_mesh_t), any float dtype
# ---------------------------------------------------------------------------------------------------------------------
def _unit(v):
    n = np.sqrt((v * v).sum(-1, keepdims=True))
    return v / np.where(n > 0, n, 1), n[..., 0]


def shade(mesh, T, face, bary, sh, dtype=np.float64):
    """mesh: dict verts (V,3), colors, normals, uvs or None, tex (TH,TW,>=3) or None, faces (F,3) of ONE object; T (4,4);
    face (...,) ids >= 0, bary (...,3) -> rgb (...,3).  sh: dict ambient diffuse specular shininess light (3) light_frame smooth
    quantize.  Evaluated in `dtype` throughout (float32: the reference's own rounding, for the colour floor)."""
    c = lambda a: np.asarray(a, dtype)
    tri = np.asarray(mesh['faces'])[face]                                    # (...,3)
    b = c(bary)
    R, tr = c(T[:3, :3]), c(T[:3, 3])
    Pc = c(mesh['verts']) @ R.T + tr                                         # camera frame
    A, B, C = Pc[tri[..., 0]], Pc[tri[..., 1]], Pc[tri[..., 2]]
    interp = lambda a: b[..., 0:1] * a[tri[..., 0]] + b[..., 1:2] * a[tri[..., 1]] + b[..., 2:3] * a[tri[..., 2]]
    l = c(sh['light'])
    if sh['light_frame'] == 1:
        l = R @ l
    if sh['smooth']:
        n, _ = _unit(interp(c(mesh['normals'])) @ R.T)
        lam = np.maximum((n * l).sum(-1), 0)
    else:
        n, nn = _unit(np.cross(B - A, C - A))
        lam = np.where(nn > 0, np.abs((n * l).sum(-1)), 0)
    shd = c(sh['ambient']) + c(sh['diffuse']) * lam
    spec = np.zeros_like(lam)
    if sh['specular'] > 0:
        pos = b[..., 0:1] * A + b[..., 1:2] * B + b[..., 2:3] * C
        view, _ = _unit(-pos)
        hv, hn = _unit(l + view)
        nh = (n * hv).sum(-1)
        if not sh['smooth']:
            nh = np.abs(nh)
        ok = (lam > 0) & (nh > 0) & (hn > 0)
        spec = np.where(ok, c(sh['specular']) * np.power(np.where(ok, nh, 1), c(sh['shininess'])), 0).astype(dtype)
    texel = np.ones(b.shape[:-1] + (3,), dtype)
    if mesh.get('tex') is not None and mesh.get('uvs') is not None:
        tex = c(mesh['tex'])[..., :3]
        TH, TW = tex.shape[:2]
        uv = interp(c(mesh['uvs']))
        uv = uv - np.floor(uv)                                               # repeat wrap
        gx, gy = uv[..., 0] * TW - c(0.5), uv[..., 1] * TH - c(0.5)          # texel centres at (i + 0.5) / size
        ix, iy = np.floor(gx), np.floor(gy)
        ax, ay = (gx - ix)[..., None], (gy - iy)[..., None]
        ix, iy = ix.astype(np.int64), iy.astype(np.int64)
        x0, x1, y0, y1 = ix % TW, (ix + 1) % TW, iy % TH, (iy + 1) % TH
        texel = (1 - ay) * ((1 - ax) * tex[y0, x0] + ax * tex[y0, x1]) + ay * ((1 - ax) * tex[y1, x0] + ax * tex[y1, x1])
    col = interp(c(mesh['colors'])) * texel * shd[..., None] + spec[..., None]
    col = np.clip(col, 0, 1)
    if sh['quantize']:
        col = np.floor(col * c(255) + c(0.5)) / c(255)
    return col.astype(dtype)


# ---------------------------------------------------------------------------------------------------------------------
# per-crop reference with the comparability masks and the conditioning term
# ---------------------------------------------------------------------------------------------------------------------
def _tri_terms(P, faces, K):
    """per face, from the float64 triangle: cond = S L / |A| * dz / z_min, geo = S L / |A|, width = |A| / L, near flag"""
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    T = P[np.asarray(faces)]                                                  # (F,3,3)
    z = T[..., 2]
    near = (z <= NEAR).any(1)
    zs = np.where(z > 1e-9, z, np.nan)
    ru, rv = fx * T[..., 0] / zs, fy * T[..., 1] / zs
    u, v = ru + cx, rv + cy
    S = np.abs(np.nan_to_num(np.stack([ru, rv, u, v], -1), nan=np.inf)).max(axis=(1, 2))
    e = np.stack([np.hypot(u[:, i] - u[:, j], v[:, i] - v[:, j]) for i, j in ((0, 1), (1, 2), (2, 0))], 1)
    L = e.max(1)
    A = np.abs((u[:, 1] - u[:, 0]) * (v[:, 2] - v[:, 0]) - (v[:, 1] - v[:, 0]) * (u[:, 2] - u[:, 0]))
    with np.errstate(divide='ignore', invalid='ignore'):
        geo = S * L / A
        cond = geo * (z.max(1) - z.min(1)) / z.min(1)
        width = A / L
    return dict(cond=cond, geo=geo, width=width, near=near)


def reference_crop(mesh, T, K, H, W, sh):
    """Everything the comparison needs about one crop, from float64 alone."""
    T64, K64 = np.asarray(T, np.float64), np.asarray(K, np.float64)
    faces = np.asarray(mesh['faces'])
    P = np.asarray(mesh['verts'], np.float64) @ T64[:3, :3].T + T64[:3, 3]
    depth, face, bary = cast(P, faces, K64, H, W)
    hit = face >= 0
    all_hit, all_miss = hit.all(0), (~hit).all(0)
    with np.errstate(invalid='ignore'):
        span_ok = (depth.max(0) - depth.min(0)) <= DEPTH_SPAN * depth.min(0)
    depth_cmp = all_miss | (all_hit & span_ok)
    same_face = all_hit & (face == face[0]).all(0)
    colour_cmp = (depth_cmp & all_hit) if sh['smooth'] else same_face
    terms = _tri_terms(P, faces, K64)
    f0 = np.where(hit[0], face[0], 0)
    rgb5 = np.zeros((5, H, W, 3))
    for s in range(5):
        fs = np.where(hit[s], face[s], 0)
        rgb5[s] = np.where(hit[s][..., None], shade(mesh, T64, fs, bary[s], dict(sh, quantize=0)), 0)
    rgb64 = np.where(hit[0][..., None], shade(mesh, T64, f0, bary[0], sh), 0)
    rgb32 = np.where(hit[0][..., None], shade(mesh, T64, f0, bary[0], sh, np.float32).astype(np.float64), 0)
    rgb32_raw = np.where(hit[0][..., None], shade(mesh, T64, f0, bary[0], dict(sh, quantize=0), np.float32).astype(np.float64), 0)
    # colour range of the winning triangle: at its three vertices, and what the five samples see inside it
    eye = np.eye(3)
    cv = np.stack([shade(mesh, T64, np.arange(len(faces)), np.broadcast_to(eye[k], (len(faces), 3)), dict(sh, quantize=0)) for k in range(3)])
    vrange = (cv.max(0) - cv.min(0)).max(-1)                                      # (F,)
    grad = np.abs(rgb5[1:] - rgb5[0]).max((0, 3)) / DELTA                          # per pixel, colour per px
    crange = np.maximum(vrange[f0], grad * np.nan_to_num(terms['width'][f0], posinf=0.0))
    return dict(depth=np.where(hit[0], depth[0], 0.0), face=np.where(hit[0], face[0], -1), hit=hit[0], depth_cmp=depth_cmp,
                colour_cmp=colour_cmp & hit[0], cond=terms['cond'][f0], geo=terms['geo'][f0], crange=crange, near_face=terms['near'],
                rgb=rgb64, rgb32=rgb32, rgb_raw=rgb5[0], rgb32_raw=rgb32_raw)


# ---------------------------------------------------------------------------------------------------------------------
# the case matrix
# ---------------------------------------------------------------------------------------------------------------------
def _light(v):
    v = np.asarray(v, np.float64)
    return tuple(float(x) for x in v / np.linalg.norm(v))


FLAT = dict(ambient=0.6, diffuse=0.4, specular=0.0, shininess=1.0, light_dir=_light((0.0, 0.0, -1.0)), light_frame='camera', smooth=False, quantize=False)
FLAT_OBJ = dict(ambient=0.35, diffuse=0.65, specular=0.0, shininess=1.0, light_dir=_light((0.5, -0.3, 0.8)), light_frame='object', smooth=False, quantize=False)
FLAT_SPEC = dict(ambient=0.4, diffuse=0.5, specular=0.2, shininess=12.0, light_dir=_light((0.2, 0.3, -0.9)), light_frame='camera', smooth=False, quantize=False)
SMOOTH = dict(ambient=0.3, diffuse=0.7, specular=0.0, shininess=1.0, light_dir=_light((0.4, 0.6, -0.7)), light_frame='camera', smooth=True, quantize=False)
SMOOTH_OBJ = dict(ambient=0.3, diffuse=0.7, specular=0.0, shininess=1.0, light_dir=_light((0.6, -0.5, 0.6)), light_frame='object', smooth=True, quantize=False)
RICH = dict(ambient=0.4, diffuse=0.6, specular=0.15, shininess=24.0, light_dir=_light((0.3, 0.2, 0.9)), light_frame='object', smooth=True, quantize=False)
OPENGL = dict(RICH, quantize=True)


def _box(ex, ey, ez, c=(0, 0, 0)):
    v = np.array([[sx * ex, sy * ey, sz * ez] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float32) + np.asarray(c, np.float32)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], np.int32)
    return v, f


def _octa():
    v = np.array([[0.1, 0, 0], [-0.1, 0, 0], [0, 0.08, 0], [0, -0.08, 0], [0, 0, 0.12], [0, 0, -0.12]], np.float32)
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)
    return v, f


def _sph_uv(v):
    d = v / np.linalg.norm(v, axis=1, keepdims=True)
    return np.stack([np.arctan2(d[:, 1], d[:, 0]) / (2 * np.pi) + 0.5, np.arccos(np.clip(d[:, 2], -1, 1)) / np.pi], 1).astype(np.float32)


def _textures(n, TH=32, TW=64):
    rs = np.random.RandomState(3)
    yy, xx = np.mgrid[0:TH, 0:TW]
    tex = np.stack([np.stack([0.5 + 0.5 * np.sin(xx * (0.2 + 0.1 * o) + k) * np.cos(yy * 0.3 + o) for k in range(3)], -1) for o in range(n)])
    return (0.2 + 0.8 * tex * rs.uniform(0.6, 1.0, (n, 1, 1, 3))).astype(np.float32)


def _K(B, fx, fy, cx, cy):
    return np.tile(np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32), (B, 1, 1))


class Case:
    """One row of the matrix: an object set, a batch of crops and a shading.  kind: 'object' (the caps hold), 'black'
    (nothing may be drawn), 'near' (the near-rule exemption dominates), 'tie' (exact ties)."""

    def __init__(self, name, verts, faces, colors, obj, TCO, K, H, W, shading, kind='object', textured=False, well_conditioned=False):
        self.name, self.verts, self.faces, self.colors = name, verts, faces, colors
        self.obj = np.asarray(obj, np.int32); self.TCO = np.asarray(TCO, np.float32); self.K = np.asarray(K, np.float32)
        self.H, self.W, self.shading, self.kind, self.well_conditioned = H, W, dict(shading), kind, well_conditioned
        self.labels = np.array([f'obj_{i:03d}' for i in range(len(verts))])
        self.uvs = [_sph_uv(v) for v in verts] if textured else None
        self.tex = _textures(len(verts)) if textured else None
        self.B = len(self.obj)

    def meshes(self):
        """the project's own padded object set (host tensors; .cuda() for the GPU tests)"""
        from cosypose_amd.rasterizer import RenderMeshes
        return RenderMeshes(self.labels, self.verts, self.faces, self.colors, uvs_list=self.uvs, textures=self.tex)

    def infos(self):
        return [dict(name=self.labels[o]) for o in self.obj]

    @functools.cached_property
    def light32(self):
        """the unit light as the float32 triple every side gets (HipBatchRenderer normalises in float64 and stores float32)"""
        l = np.asarray(self.shading['light_dir'], np.float64)
        return (l / np.linalg.norm(l)).astype(np.float32)

    def shade_dict(self):
        s = self.shading
        return dict(ambient=np.float32(s['ambient']), diffuse=np.float32(s['diffuse']), specular=np.float32(s['specular']),
                    shininess=np.float32(s['shininess']), light=self.light32, light_frame=1 if s['light_frame'] == 'object' else 0,
                    smooth=int(bool(s['smooth'])), quantize=int(bool(s['quantize'])))

    def object_arrays(self, m, o):
        nf = int(m.n_faces[o])
        d = dict(verts=m.verts[o].numpy(), colors=m.colors[o].numpy(), normals=m.normals[o].numpy(), faces=m.faces[o].numpy()[:nf], uvs=None, tex=None)
        if m.tex is not None:
            d['uvs'], d['tex'] = m.uvs[o].numpy(), m.tex[o].numpy()
        return d

    @functools.cached_property
    def reference(self):
        """list over crops of reference_crop(...) dicts; crops with a non-finite pose or camera: None (black by contract)"""
        m = self.meshes()
        out = []
        for b in range(self.B):
            if not (np.isfinite(self.TCO[b]).all() and np.isfinite(self.K[b]).all()):
                out.append(None)
                continue
            out.append(reference_crop(self.object_arrays(m, self.obj[b]), self.TCO[b], self.K[b], self.H, self.W, self.shade_dict()))
        return out

    def twin(self, oracle):
        """oracle.rasterize on this case -> rgb (B,3,H,W), depth (B,H,W), face ids (B,H,W) (-1 = background)"""
        m, s = self.meshes(), self.shade_dict()
        kw = dict(normals=m.normals.numpy())
        if m.tex is not None:
            kw.update(uvs=m.uvs.numpy(), tex=m.tex.numpy())
        rgb, depth, zb = oracle.rasterize(m.verts.numpy(), m.colors.numpy(), m.faces.numpy(), m.n_faces.numpy(), self.obj, self.TCO, self.K,
                                          self.H, self.W, ambient=s['ambient'], diffuse=s['diffuse'], light_dir=tuple(self.light32),
                                          specular=s['specular'], shininess=s['shininess'], light_frame=s['light_frame'], smooth=s['smooth'],
                                          quantize=s['quantize'], **kw)
        face = np.where(zb == np.uint64(0xFFFFFFFFFFFFFFFF), -1, (zb & np.uint64(0xFFFFFFFF)).astype(np.int64))
        return rgb, depth, face


def _fan_disc(n=40, r=0.15, needle=0.00007):
    """a disc of n wide and n needle triangles around its centre: the needles are interior (no silhouette of their own), r long
    and `needle` wide at the rim; seen at ~1000 px per metre they are 150 px by 0.07 px"""
    ang = np.linspace(0, 2 * np.pi, n, endpoint=False) + 0.0123
    v = [[0, 0, 0]]
    for a in ang:
        v.append([r * np.cos(a), r * np.sin(a), 0])
        d = needle / r
        v.append([r * np.cos(a + d), r * np.sin(a + d), 0])
    v = np.asarray(v, np.float32)
    f = []
    for k in range(n):
        a, b, c = 1 + 2 * k, 2 + 2 * k, 1 + 2 * ((k + 1) % n)
        f += [(0, a, b), (0, b, c)]
    return v, np.asarray(f, np.int32)


def _tie_mesh():
    """four triangles around a centre vertex, every face with vertices of its own (distinct colours: the colour names the face).
    With K = [[64,0,32],[0,64,32]] and TCO = identity + (0,0,1) vertex (x,y,0) lands on pixel coordinate 64 x + 32 exactly: the
    centre on the pixel centre (20.5, 20.5), the corners on (4.5,4.5) (36.5,4.5) (36.5,36.5) (4.5,36.5); the four shared
    edges are the diagonals, through pixel centres.  Every triangle's edge-function area is 32 * 16 = 2^9: the barycentrics are exact
    in float32, they sum to exactly 1, the depth is exactly 1 and a face of one colour (entries 1 and 0.25) renders exactly that colour."""
    g = lambda px, py: [(px - 32) / 64, (py - 32) / 64, 0.0]
    c, k = g(20.5, 20.5), [g(4.5, 4.5), g(36.5, 4.5), g(36.5, 36.5), g(4.5, 36.5)]
    v, f = [], []
    for i in range(4):
        f.append([len(v), len(v) + 1, len(v) + 2]); v += [c, k[i], k[(i + 1) % 4]]
    col = np.repeat(np.array([[1.0, 0.25, 0.25], [0.25, 1.0, 0.25], [0.25, 0.25, 1.0], [1.0, 1.0, 0.25]], np.float32), 3, axis=0)
    return np.asarray(v, np.float32), np.asarray(f, np.int32), col


def _rand_colors(seed, verts):
    rs = np.random.RandomState(seed)
    return [rs.uniform(0.2, 1.0, (len(v), 3)).astype(np.float32) for v in verts]


def _build_cases():
    from cosypose_amd import synthetic as syn
    v5, f5, c5 = syn.make_render_meshes(7, 5)
    cases = []
    add = lambda *a, **k: cases.append(Case(*a, **k))
    add('usual_240x320', v5, f5, c5, [0, 1, 2, 3, 4], syn.make_TCO(11, 5, z_range=(0.5, 1.0), xy=0.05), _K(5, 520., 515., 158.3, 121.7), 240, 320, FLAT,
        well_conditioned=True)
    add('b1', v5, f5, c5, [2], syn.make_TCO(12, 1, z_range=(1.2, 1.5), xy=0.02), _K(1, 520., 515., 63.3, 48.7), 96, 128, SMOOTH)
    add('b17', v5, f5, c5, np.arange(17) % 5, syn.make_TCO(13, 17, z_range=(2.5, 4.0), xy=0.03), _K(17, 520., 515., 31.7, 24.3), 48, 64, FLAT_OBJ)
    # three small objects, then two close-ups that fill the frame: pixel 0 and the last pixel of a crop are foreground, so a resolve
    # pass that runs one pixel past H * W (45 * 61 is not a multiple of the 256-thread block) changes what the neighbours hold
    Ts = np.concatenate([syn.make_TCO(14, 3, z_range=(2.5, 3.5), xy=0.02), syn.make_TCO(26, 2, z_range=(0.25, 0.3), xy=0.0)])
    add('size_45x61', v5, f5, c5, [0, 3, 4, 1, 2], Ts, _K(5, 520., 515., 30.2, 22.9), 45, 61, OPENGL, textured=True)
    add('size_48x64', v5, f5, c5, [0, 3, 4, 1, 2], Ts, _K(5, 520., 515., 31.7, 24.3), 48, 64, OPENGL, textured=True)
    add('far', v5, f5, c5, [0, 1, 4], syn.make_TCO(15, 3, z_range=(3.0, 6.0), xy=0.3), _K(3, 520., 515., 79.3, 60.7), 120, 160, FLAT_SPEC)
    add('close_offscreen', v5, f5, c5, [1, 2, 3], syn.make_TCO(16, 3, z_range=(0.15, 0.3), xy=0.08), _K(3, 400., 398., 63.3, 48.7), 96, 128, RICH, textured=True)
    T = syn.make_TCO(17, 2, z_range=(0.8, 1.0), xy=0.02); T[0, 0, 3] = 2.0; T[1, 1, 3] = -1.5
    add('offscreen', v5, f5, c5, [0, 1], T, _K(2, 210., 208., 63.3, 48.7), 96, 128, FLAT, kind='black')
    add('near_plane', v5, f5, c5, [0, 1, 2, 3], syn.make_TCO(18, 4, z_range=(0.02, 0.12), xy=0.01), _K(4, 210., 208., 63.3, 48.7), 96, 128, FLAT, kind='near')
    T = syn.make_TCO(19, 3, z_range=(1.0, 1.4), xy=0.02)
    T[:, 0, 3] += T[:, 2, 3] * (400 + 64) / 520; T[:, 1, 3] += T[:, 2, 3] * (48 - 700) / 515
    add('pp_outside', v5, f5, c5, [0, 2, 4], T, _K(3, 520., 515., -400., 700.), 96, 128, SMOOTH_OBJ)
    add('f2600', v5, f5, c5, [1, 3], syn.make_TCO(20, 2, z_range=(2.5, 3.5), xy=0.02), _K(2, 2600., 2600., 79.3, 60.7), 120, 160, RICH, textured=True)
    ov, of = _octa()
    cv = [_box(0.1, 0.08, 0.06)[0], _box(0.05, 0.12, 0.09)[0], ov, v5[0]]
    cf = [_box(1, 1, 1)[1], _box(1, 1, 1)[1], of, f5[0]]
    add('coarse_mixed', cv, cf, _rand_colors(5, cv[:3]) + [c5[0]], [0, 1, 2, 3, 2, 0], syn.make_TCO(21, 6, z_range=(0.45, 0.8), xy=0.03),
        _K(6, 520., 520., 64., 64.), 128, 128, FLAT_OBJ)
    (va, fa), (vb, _) = _box(0.08, 0.05, 0.05), _box(0.04, 0.09, 0.04, c=(0.03, 0.01, 0.02))
    iv, iff = [np.concatenate([va, vb])], [np.concatenate([fa, fa + 8])]
    add('interpenetrating', iv, iff, _rand_colors(6, iv), [0, 0, 0], syn.make_TCO(22, 3, z_range=(1.0, 1.4), xy=0.02), _K(3, 520., 520., 64., 48.), 96, 128, FLAT)
    nv, nf = _fan_disc()
    T = syn.make_TCO(23, 2, z_range=(1.0, 1.0), xy=0.0)
    c_, s_ = np.cos(0.5), np.sin(0.5)
    T[0, :3, :3] = np.array([[1, 0, 0], [0, c_, -s_], [0, s_, c_]]); T[1, :3, :3] = np.array([[c_, 0, s_], [0, -1, 0], [s_, 0, -c_]])
    add('needle_fan', [nv], [nf], _rand_colors(8, [nv]), [0, 0], T, _K(2, 1000., 1000., 160.4, 120.3), 240, 320, FLAT)
    pv, pf, pc = [], [], []
    for i, (nl, no) in enumerate(((24, 32), (10, 12), (16, 20))):
        a, b, c = syn.make_render_meshes(30 + i, 1, n_lat=nl, n_lon=no); pv += a; pf += b; pc += c
    add('padded_mixed_VF', pv, pf, pc, [1, 0, 2, 1], syn.make_TCO(24, 4, z_range=(1.2, 1.8), xy=0.03), _K(4, 520., 515., 63.3, 48.7), 96, 128, SMOOTH)
    T = syn.make_TCO(25, 3, z_range=(1.2, 1.8), xy=0.03); T[:, :3, 0] *= -1                       # det R = -1
    add('mirror', v5, f5, c5, [0, 2, 3], T, _K(3, 520., 515., 63.3, 48.7), 96, 128, RICH, textured=True)
    tv, tf, tc = _tie_mesh()
    T = np.tile(np.eye(4, dtype=np.float32), (1, 1, 1)); T[0, 2, 3] = 1.0
    add('exact_tie', [tv], [tf], [tc], [0], T, _K(1, 64., 64., 32., 32.), 40, 40, dict(FLAT, ambient=1.0, diffuse=0.0), kind='tie')
    return {c.name: c for c in cases}


@functools.lru_cache(maxsize=None)
def cases():
    return _build_cases()


CASE_NAMES = ['usual_240x320', 'b1', 'b17', 'size_45x61', 'size_48x64', 'far', 'close_offscreen', 'offscreen', 'near_plane', 'pp_outside', 'f2600',
              'coarse_mixed', 'interpenetrating', 'needle_fan', 'padded_mixed_VF', 'mirror', 'exact_tie']


# ---------------------------------------------------------------------------------------------------------------------
# the rules
# ---------------------------------------------------------------------------------------------------------------------
def float32_floor(case):
    """worst |float32 evaluation - float64 evaluation| of shade() at the float64 hit points, over the colour-comparable pixels"""
    w = 0.0
    for r in case.reference:
        if r is not None and r['colour_cmp'].any():
            w = max(w, float(np.abs(r['rgb32_raw'][r['colour_cmp']] - r['rgb_raw'][r['colour_cmp']]).max()))
    return w


def compare(case, rgb, depth, face, who):
    """Hold a render of `case` -- rgb (B,3,H,W), depth (B,H,W), winning face ids (B,H,W) (-1 background) of the twin or the
    kernel -- to the reference under the rules of the module docstring.  Prints the figures, asserts, returns them."""
    ref = case.reference
    n_fg = n_exempt = n_cmp_fg = n_near = n_col = 0
    worst_d = worst_c = 0.0
    bounds, flips, flips32, nq = [], 0, 0, 0
    floor = FLOOR[case.name]
    quant = bool(case.shading['quantize'])
    for b, r in enumerate(ref):
        if r is None:
            assert (rgb[b] == 0).all() and (depth[b] == 0).all(), (case.name, b, 'non-finite pose must be black')
            continue
        got_hit = depth[b] > 0
        fg = r['hit'] | got_hit
        got_near = got_hit & r['near_face'][np.maximum(face[b], 0)]
        # the whole-triangle rule itself: the rasteriser never draws a triangle that has a vertex at or before the near plane
        assert not got_near.any(), (case.name, who, b, 'drew a triangle with a vertex at z <= 0.01', int(got_near.sum()))
        near = (r['hit'] & r['near_face'][np.maximum(r['face'], 0)]) | got_near
        cmp_d = r['depth_cmp'] & ~near
        n_fg += int(fg.sum()); n_near += int((fg & near).sum()); n_exempt += int((fg & ~cmp_d).sum())
        # foreground / background decision: equal on every depth-comparable pixel, no tolerance
        bad = cmp_d & (got_hit != r['hit'])
        assert not bad.any(), (case.name, who, b, 'foreground/background differs on comparable pixels', int(bad.sum()), np.argwhere(bad)[:5].tolist())
        m = cmp_d & r['hit']
        n_cmp_fg += int(m.sum())
        if m.any():
            bound = r['depth'][m] * EPS32 * (C0 + KAPPA * r['cond'][m])
            ratio = np.abs(depth[b][m].astype(np.float64) - r['depth'][m]) / bound
            worst_d = max(worst_d, float(ratio.max()))
            bounds.append(bound / r['depth'][m])
        mc = r['colour_cmp'] & ~near & got_hit
        if mc.any():
            n_col += int(mc.sum())
            g = rgb[b].transpose(1, 2, 0)[mc].astype(np.float64)
            cb = EPS32 * KAPPA * r['geo'][mc] * r['crange'][mc] + floor
            if quant:
                # judged before rounding: the kernel's value lies within the bound of the unrounded reference, up to the half step
                d = np.abs(g - r['rgb'][mc])
                assert d.max() <= 1 / 255 + 1e-6, (case.name, who, b, 'more than one 8-bit step', float(d.max()))
                flips += int((d > 0.5 / 255).sum()); flips32 += int((np.abs(r['rgb32'][mc] - r['rgb'][mc]) > 0.5 / 255).sum()); nq += d.size
                near_step = np.abs(r['rgb_raw'][mc] * 255 + 0.5 - np.round(r['rgb_raw'][mc] * 255 + 0.5)) / 255
                # a flipped value must be one whose unrounded reference sits within the bound of a rounding threshold
                ok = (d <= 0.5 / 255) | (near_step <= cb[:, None])
                worst_c = max(worst_c, float((np.where(d > 0.5 / 255, near_step, 0) / cb[:, None]).max()))
                assert ok.all(), (case.name, who, b, 'a step of difference away from any rounding threshold', int((~ok).sum()))
            else:
                dc = np.abs(g - r['rgb'][mc]).max(-1)
                with np.errstate(divide='ignore', invalid='ignore'):
                    ratio = np.where(dc == 0, 0.0, dc / cb)              # (exact_tie: bound 0, deviation 0)
                worst_c = max(worst_c, float(ratio.max()))
    med = float(np.median(np.concatenate(bounds))) if bounds else 0.0
    share = n_exempt / max(n_fg, 1)
    fig = dict(case=case.name, who=who, foreground=n_fg, exempt=n_exempt, exempt_share=share, near_exempt=n_near, comparable_fg=n_cmp_fg,
               colour_cmp=n_col, depth_ratio=worst_d, colour_ratio=worst_c, median_bound=med, flips=flips, flips32=flips32, nq=nq)
    print(f'  {case.name:18s} {who:6s} fg {n_fg:6d} exempt {n_exempt:5d} ({share:.2e}; near {n_near}) cmp {n_cmp_fg:6d} col {n_col:6d}  '
          f'depth ratio {worst_d:.3f} colour ratio {worst_c:.3f} median bound {med:.2e}' + (f' flips {flips}/{nq} (float32 ref {flips32})' if quant else ''))
    assert worst_d <= 1.0, (case.name, who, 'depth outside the bound', worst_d)
    assert worst_c <= 1.0, (case.name, who, 'colour outside the bound', worst_c)
    if quant:
        assert flips <= flips32, (case.name, who, 'more one-step flips than the float32 reference shows', flips, flips32, nq)
    if case.kind == 'object':
        assert share <= 0.01, (case.name, who, 'exempt share', share)
        assert n_cmp_fg >= 100, (case.name, who, 'comparable foreground', n_cmp_fg)
    if case.kind == 'near':
        # the foreground is dominated by triangles at or beyond z = 0.01: the exemptions must be THAT reason, and the rest must hold
        assert n_near >= 1000 and n_exempt - n_near <= 0.01 * n_fg and n_cmp_fg >= 100, (case.name, who, NEAR_REASON, n_near, n_exempt, n_fg, n_cmp_fg)
    if case.kind == 'black':
        assert n_fg == 0 and not rgb.any() and not depth.any(), (case.name, who, 'must be black')
    if case.well_conditioned:
        assert med < 2e-6, (case.name, 'median depth bound', med)
    return fig
