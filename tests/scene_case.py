"""Case matrix and the two references of the scene renderer (cosypose_amd/scene_renderer.py, csrc/kernels_scene.hip).  A helper module
(like raster_ref.py / ransac_case.py), numpy only on the reference side.

TWIN COMPOSITE.  oracle.rasterize -- the CPU twin of the batch rasteriser, the same float32 arithmetic in scalar loops -- once per view
with B = the view's rows (K tiled), composed on the host lexicographically on (depth bits, row order in the call, face id): the
z-buffer key of the kernel spelled out.  Gives the expected rgb, depth, mask, pixel counts and boxes; a row's silhouette is its own
z-buffer.  A row with a colour override is rasterised as an extra object: the same mesh with every vertex colour set to that rgb.
The kernel must equal this bit for bit.

FLOAT64 COMPOSITE.  raster_ref.cast (ray casting, no image-plane arithmetic) per row at the pixel centre and at raster_ref's four
sub-pixel offsets; the nearest hit per pixel over the view's rows.  The mask must agree with it outside the EXEMPT pixels:
  * the two nearest float64 depths of the pixel, each the nearest hit of another row of the view, differ by less than 1e-4 m (which of two
    faces of ONE row is in front does not enter the mask), or
  * a row's hit / miss state differs between the sub-pixel offsets (a silhouette runs within 2^-10 px of the pixel centre).
A row that repeats an earlier row of its view exactly (same object, same pose bits) is the same surface and does not enter: the tie rule
gives every pixel to the earlier row.
Exempt pixels may make up at most 2 % of a view's foreground (EXEMPT_CAP): a condition on the cases, not a measurement -- the base
scene has none.  Apart from those, raster_ref's NEAR rule: the rasteriser drops a triangle with a vertex at z <= 0.01 whole where the
ray caster (like OpenGL) clips it per pixel, so pixels whose float64 winner is such a triangle are exempt for that reason and counted
separately (only the near-plane case has any).
"""
import functools

import numpy as np

import raster_ref as R

MISS = np.uint64(0xFFFFFFFFFFFFFFFF)
DEPTH_TIE = 1e-4          # metres
EXEMPT_CAP = 0.02


class SceneCase:
    def __init__(self, name, verts, faces, colors, obj, view, TCO, K, H, W, shading=R.FLAT, shading_name='flat', row_colors=None,
                 background=(0, 0, 0), tie=False):
        self.name, self.verts, self.faces, self.vcolors = name, list(verts), list(faces), list(colors)
        self.obj, self.view = np.asarray(obj, np.int32), np.asarray(view, np.int32)
        self.TCO, self.K = np.asarray(TCO, np.float32), np.asarray(K, np.float32)
        self.H, self.W, self.shading, self.shading_name = H, W, dict(shading), shading_name
        self.row_colors = None if row_colors is None else np.asarray(row_colors, np.float32)
        self.background, self.tie = tuple(background), tie
        self.labels = np.array([f'obj_{i:03d}' for i in range(len(self.verts))])
        self.N, self.n_views = len(self.obj), len(self.K)
        assert self.TCO.shape == (self.N, 4, 4) and len(self.view) == self.N

    # ---- the object set
    def meshes(self):
        from cosypose_amd.rasterizer import RenderMeshes
        return RenderMeshes(self.labels, self.verts, self.faces, self.vcolors)

    @functools.cached_property
    def _flat(self):
        """(verts, faces, colors lists, obj per row) with one extra uniformly coloured object per overridden row"""
        v, f, c, obj = list(self.verts), list(self.faces), list(self.vcolors), self.obj.copy()
        if self.row_colors is not None:
            for r in np.flatnonzero(self.row_colors[:, 3] >= 0):
                obj[r] = len(v)
                v.append(self.verts[self.obj[r]]); f.append(self.faces[self.obj[r]])
                c.append(np.tile(self.row_colors[r, :3], (len(self.verts[self.obj[r]]), 1)).astype(np.float32))
        return v, f, c, obj

    def flat_meshes(self):
        """the object set in which the colour overrides are real vertex colours, and the rows' objects in it"""
        from cosypose_amd.rasterizer import RenderMeshes
        v, f, c, obj = self._flat
        return RenderMeshes(np.array([f'obj_{i:03d}' for i in range(len(v))]), v, f, c), obj

    @property
    def row_labels(self):
        return self.labels[self.obj]

    @functools.cached_property
    def background32(self):
        return np.asarray(self.background, np.float32) / np.float32(255.0)

    def finite(self, r):
        return bool(np.isfinite(self.TCO[r]).all() and np.isfinite(self.K[self.view[r]]).all())

    def with_rows(self, name, rows, **over):
        """the same scene with a subset / another order of the rows"""
        rows = np.asarray(rows)
        kw = dict(shading=self.shading, shading_name=self.shading_name, row_colors=None if self.row_colors is None else self.row_colors[rows],
                  background=self.background, tie=self.tie)
        kw.update(over)
        return SceneCase(name, self.verts, self.faces, self.vcolors, self.obj[rows], self.view[rows], self.TCO[rows], self.K, self.H, self.W, **kw)


def shade_kwargs(shading):
    l = np.asarray(shading['light_dir'], np.float64)
    return dict(ambient=np.float32(shading['ambient']), diffuse=np.float32(shading['diffuse']), light_dir=tuple((l / np.linalg.norm(l)).astype(np.float32)),
                specular=np.float32(shading['specular']), shininess=np.float32(shading['shininess']), light_frame=1 if shading['light_frame'] == 'object' else 0,
                smooth=int(bool(shading['smooth'])), quantize=int(bool(shading['quantize'])))


def _boxes(sets, N):
    out = np.full((N, 4), -1.0, np.float32)
    for r, s in enumerate(sets):
        if s is not None and s.any():
            ys, xs = np.nonzero(s)
            out[r] = (xs.min(), ys.min(), xs.max(), ys.max())
    return out


_TWIN = {}


def twin_composite(case, oracle):
    """-> dict rgb (n_views,3,H,W), depth, mask (n_views,H,W), px_count_all, px_count_visib (N,), visib_fract (N,) float32, bbox_obj,
    bbox_visib (N,4) float32: what the kernel must give, bit for bit.  Computed once per case and shared; treat as read-only."""
    if case.name in _TWIN:
        return _TWIN[case.name]
    m, obj = case.flat_meshes()
    kw = dict(shade_kwargs(case.shading), normals=m.normals.numpy())
    H, W, N = case.H, case.W, case.N
    rgb = np.empty((case.n_views, 3, H, W), np.float32); rgb[:] = case.background32[None, :, None, None]
    depth = np.zeros((case.n_views, H, W), np.float32); mask = np.full((case.n_views, H, W), -1, np.int32)
    sil = [None] * N
    for v in range(case.n_views):
        rows = np.flatnonzero(case.view == v)                        # call order
        if not len(rows):
            continue
        r_rgb, r_depth, zb = oracle.rasterize(m.verts.numpy(), m.colors.numpy(), m.faces.numpy(), m.n_faces.numpy(), obj[rows], case.TCO[rows],
                                              np.tile(case.K[v], (len(rows), 1, 1)), H, W, **kw)
        best = np.full((H, W), 1 << 32, np.uint64)
        for j, r in enumerate(rows):
            hit = zb[j] != MISS
            sil[r] = hit
            bits = zb[j] >> np.uint64(32)
            take = hit & (bits < best)                               # strict: at equal depth bits the row that comes first stays
            best[take] = bits[take]; mask[v][take] = r; depth[v][take] = r_depth[j][take]
            rgb[v][:, take] = r_rgb[j][:, take]
    visib = [mask[case.view[r]] == r for r in range(N)]
    n_all = np.array([0 if s is None else int(s.sum()) for s in sil], np.int32)
    n_vis = np.array([int(s.sum()) for s in visib], np.int32)
    with np.errstate(divide='ignore', invalid='ignore'):
        fract = np.where(n_all > 0, n_vis.astype(np.float32) / np.maximum(n_all, 1).astype(np.float32), np.float32(0)).astype(np.float32)
    out = dict(rgb=rgb, depth=depth, mask=mask, px_count_all=n_all, px_count_visib=n_vis, visib_fract=fract, bbox_obj=_boxes(sil, N),
               bbox_visib=_boxes(visib, N), silhouettes=sil)
    _TWIN[case.name] = out
    return out


_CAST = {}


def _cast_row(verts, faces, T, K, H, W):
    """raster_ref.cast of one row, cached by content: the variants of the base scene share their rows
    -> (depth (S,H,W), near (H,W): the centre sample's winning triangle has a vertex at z <= 0.01)"""
    key = (verts.tobytes(), faces.tobytes(), T.tobytes(), K.tobytes(), H, W)
    if key not in _CAST:
        P = verts.astype(np.float64) @ T[:3, :3].astype(np.float64).T + T[:3, 3].astype(np.float64)
        Kd = K.astype(np.float64)
        d, f, _ = R.cast(P, faces, Kd, H, W)
        near_face = P[faces][:, :, 2].min(1) <= R.NEAR
        near = (f[0] >= 0) & near_face[np.maximum(f[0], 0)]
        _CAST[key] = (d, near)
    return _CAST[key]


_F64 = {}


def float64_composite(case):
    """-> dict mask (n_views,H,W) (nearest float64 hit at the pixel centre, -1 = miss), exempt, near (n_views,H,W) bool, foreground
    (n_views,H,W) bool.  Computed once per case and shared; treat as read-only."""
    if case.name in _F64:
        return _F64[case.name]
    m = case.meshes()
    H, W = case.H, case.W
    mask = np.full((case.n_views, H, W), -1, np.int32)
    exempt = np.zeros((case.n_views, H, W), bool); near = np.zeros_like(exempt)
    for v in range(case.n_views):
        rows, seen = [], set()
        for r in np.flatnonzero(case.view == v):
            # a row that repeats an earlier row of the view exactly (same object, same pose bits) is the same surface: by the tie rule the
            # earlier row wins every pixel, and the depth-tie exemption is about two DIFFERENT surfaces
            key = (int(case.obj[r]), case.TCO[r].tobytes())
            if case.finite(r) and key not in seen:
                seen.add(key); rows.append(r)
        if not rows:
            continue
        d0 = np.full((len(rows), H, W), np.inf); nr = np.zeros((len(rows), H, W), bool)
        for j, r in enumerate(rows):
            o = case.obj[r]
            d, n = _cast_row(m.verts[o].numpy(), m.faces[o].numpy()[:int(m.n_faces[o])], case.TCO[r], case.K[v], H, W)
            hit = np.isfinite(d)
            exempt[v] |= hit.any(0) != hit.all(0)                   # the row's hit / miss state differs between the offsets
            d0[j], nr[j] = d[0], n
        order = np.argsort(d0, axis=0, kind='stable')               # equal depths: the row that comes first
        first = np.take_along_axis(d0, order[:1], 0)[0]
        win = order[0]
        fg = np.isfinite(first)
        mask[v][fg] = np.asarray(rows)[win[fg]]
        if len(rows) > 1:
            second = np.take_along_axis(d0, order[1:2], 0)[0]
            with np.errstate(invalid='ignore'):
                exempt[v] |= fg & np.isfinite(second) & (second - first < DEPTH_TIE)
        near[v] = fg & np.take_along_axis(nr, order[:1], 0)[0]
    out = dict(mask=mask, exempt=exempt, near=near, foreground=mask >= 0)
    _F64[case.name] = out
    return out


def compare_masks(case, mask, who):
    """`mask` (n_views,H,W) of the twin composite or the kernel against the float64 composite under the module's rule.  Prints the
    figures, asserts, returns them per view."""
    ref = float64_composite(case)
    figs = []
    for v in range(case.n_views):
        fg = ref['foreground'][v] | (mask[v] >= 0)
        ex = ref['exempt'][v] & fg & ~ref['near'][v]
        skip = ref['exempt'][v] | ref['near'][v]
        bad = (mask[v] != ref['mask'][v]) & ~skip
        n_fg, n_ex, n_near, n_bad = int(fg.sum()), int(ex.sum()), int((ref['near'][v] & fg).sum()), int(bad.sum())
        print(f'  {case.name:18s} {who:6s} view {v}: foreground {n_fg:5d} exempt {n_ex:4d} near-exempt {n_near:4d} mismatches {n_bad}')
        assert n_ex <= EXEMPT_CAP * max(n_fg, 1), (case.name, who, v, 'exempt share of the foreground', n_ex, n_fg)
        assert n_bad == 0, (case.name, who, v, 'mask differs from the float64 composite', n_bad, np.argwhere(bad)[:5].tolist())
        figs.append(dict(foreground=n_fg, exempt=n_ex, near=n_near))
    return figs


# ---------------------------------------------------------------------------------------------------------------------
# the case matrix
# ---------------------------------------------------------------------------------------------------------------------
def _K(fx, cx, cy, n=1):
    return np.tile(np.array([[fx, 0, cx], [0, fx, cy], [0, 0, 1]], np.float32), (n, 1, 1))


def _T(x, y, z, R3=None):
    T = np.eye(4)
    if R3 is not None:
        T[:3, :3] = R3
    T[:3, 3] = (x, y, z)
    return T


BASE_OBJECTS = (0, 1, 2, 3, 4, 5, 5)


def base_world():
    """the base scene in the world frame -> TWO (7,4,4) of BASE_OBJECTS, TWC (3,4,4), float64"""
    from cosypose_amd import synthetic as syn
    rs = np.random.RandomState(1)
    TWO = []
    for _ in range(6):
        T = syn._rigid_noise(rs, 2.0, 0.0)
        T[:3, 3] = (rs.uniform(-.18, .18), rs.uniform(-.18, .18), rs.uniform(0, .1))
        TWO.append(T)
    T6 = TWO[5].copy(); T6[:3, 3] += (0.05, 0.02, 0.01)             # interpenetrating boxes
    return np.stack(TWO + [T6]), syn.make_ba_scene(5, 7, 3, 8)['cam_TWC']


def _base_arrays():
    from cosypose_amd import synthetic as syn
    v, f, c = syn.make_render_meshes(7, 5)
    bv, bf = R._box(0.09, 0.06, 0.04)
    v, f, c = v + [bv], f + [bf], c + [np.full((8, 3), 0.5, np.float32)]
    TWO, TWC = base_world()
    TCO = (np.linalg.inv(TWC)[:, None] @ TWO[None]).reshape(-1, 4, 4).astype(np.float32)       # view-major, object-minor
    return v, f, c, np.tile(np.array(BASE_OBJECTS), 3), np.repeat(np.arange(3), 7), TCO


def _build_cases():
    from cosypose_amd import synthetic as syn
    from cosypose_amd.rasterizer import OPENGL_LIKE
    v, f, c, obj, view, TCO = _base_arrays()
    K3 = _K(75., 40., 30., 3)
    cases = []
    add = lambda *a, **k: cases.append(SceneCase(*a, **k))
    add('base_60x80', v, f, c, obj, view, TCO, K3, 60, 80)
    base = cases[0]
    K45 = K3.copy(); K45[:, :2] *= 0.75                              # width neither a multiple of 32 nor of 64
    add('base_45x61', v, f, c, obj, view, TCO, K45, 45, 61)
    cases.append(base.with_rows('shuffled', np.random.RandomState(4).permutation(21)))         # rows shuffled, views interleaved
    add('empty_view', v, f, c, obj, np.array([0, 2, 3])[view], TCO, _K(75., 40., 30., 4), 60, 80)   # view 1 has no row
    add('one_row', v, f, c, obj[9:10], [0], TCO[9:10], K3[:1], 60, 80)
    # the same object twice at the same pose, beside another object
    T = np.stack([_T(0.02, 0.0, 0.9, syn._rodrigues(np.random.RandomState(2), 1.0))] * 2 + [_T(-0.1, 0.05, 0.7)]).astype(np.float32)
    add('same_pose_twice', v, f, c, [1, 1, 3], [0, 0, 0], T, _K(75., 40., 30.), 60, 80, tie=True)
    # an ellipsoid wholly behind the box (17 x 11 px half extents at z = 0.4; the ellipsoid is at most 6 px at z = 2), rows in both orders
    # (the box slightly turned and shifted: its outline is not to run through pixel centres)
    Tb = _T(0.003, 0.002, 0.4, syn._rodrigues(np.random.RandomState(5), 0.1))
    T = np.stack([_T(0, 0, 2.0), Tb, Tb, _T(0, 0, 2.0)]).astype(np.float32)
    add('behind_box', v, f, c, [2, 5, 5, 2], [0, 0, 1, 1], T, _K(75., 40., 30., 2), 60, 80)
    T = np.stack([_T(5.0, 0, 1.0), _T(0.03, 0.02, 1.0), _T(0, -4.0, 0.8)]).astype(np.float32)
    add('outside_frame', v, f, c, [0, 4, 5], [0, 0, 0], T, _K(75., 40., 30.), 60, 80)
    # straddles z = 0.01 (and z = 0): the rasteriser drops its nearest triangles whole, the ray caster clips them per pixel
    T = np.stack([_T(0.1, 0.0, 0.07, syn._rodrigues(np.random.RandomState(3), 1.0)), _T(-0.05, 0.03, 0.8)]).astype(np.float32)
    add('near_plane', v, f, c, [1, 3], [0, 0], T, _K(75., 40., 30.), 60, 80)
    Tn = TCO.copy(); Tn[11, 1, 2] = np.nan
    add('nan_in_TCO', v, f, c, obj, view, Tn, K3, 60, 80)
    Kn = K3.copy(); Kn[1, 0, 2] = np.nan
    add('nan_in_K', v, f, c, obj, view, TCO, Kn, 60, 80)
    # a 12-triangle box that fills the frame (every triangle thousands of pixels: the wave-shared walk) behind one fine ellipsoid and in
    # front of another
    wv, wf = R._box(0.5, 0.4, 0.05)
    rot = syn._rodrigues(np.random.RandomState(6), 0.3)
    T = np.stack([_T(0.0, 0.0, 1.0, rot), _T(0.1, 0.05, 0.55), _T(-0.2, -0.1, 1.6)]).astype(np.float32)
    add('coarse_over_fine', [wv, v[0], v[3]], [wf, f[0], f[3]], [np.full((8, 3), 0.8, np.float32), c[0], c[3]], [0, 1, 2], [0, 0, 0], T,
        _K(75., 40., 30.), 60, 80)
    ov, of = R._octa()
    pv, pf, pc = syn.make_render_meshes(31, 1, n_lat=6, n_lon=8)
    mv, mf, mc = [ov, v[5], pv[0], v[2]], [of, f[5], pf[0], f[2]], [np.full((6, 3), 0.3, np.float32), c[5], pc[0], c[2]]
    T = syn.make_TCO(24, 6, z_range=(0.6, 1.0), xy=0.08)
    add('padded_mixed_VF', mv, mf, mc, [0, 1, 2, 3, 2, 0], [0, 0, 0, 1, 1, 1], T, _K(75., 40., 30., 2), 60, 80)
    col = np.full((21, 4), -1.0, np.float32)
    col[[1, 5, 8, 20]] = [[0.9, 0.1, 0.2, 1.0], [0.1, 0.8, 0.3, 0.0], [0.2, 0.3, 0.9, 0.5], [1.0, 1.0, 0.0, 1.0]]     # alpha 0: still an override
    add('colour_override', v, f, c, obj, view, TCO, K3, 60, 80, row_colors=col)
    add('background', v, f, c, obj, view, TCO, K3, 60, 80, background=(30, 120, 200))
    add('opengl', v, f, c, obj, view, TCO, K3, 60, 80, shading=OPENGL_LIKE, shading_name='opengl')
    return {c.name: c for c in cases}


@functools.lru_cache(maxsize=None)
def cases():
    return _build_cases()


CASE_NAMES = ['base_60x80', 'base_45x61', 'shuffled', 'empty_view', 'one_row', 'same_pose_twice', 'behind_box', 'outside_frame', 'near_plane',
              'nan_in_TCO', 'nan_in_K', 'coarse_over_fine', 'padded_mixed_VF', 'colour_override', 'background', 'opengl']
