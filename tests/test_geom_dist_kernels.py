"""Geometry, distance and loss kernels (csrc/kernels_geom.hip, csrc/kernels_dist.hip and their C ABI wrappers) against float64.

tests/test_gpu_parity.py holds these kernels at essentially one shape each (B = 6, P = 2000, or the one golden distance case), mostly
against oracle/cosy_oracle.c -- a float32 restatement written beside the kernels, which shares their reading of the reference and
their rounding.  Here the yardstick is this module's own float64 numpy restatement of the reference's Python, written from the
reference's text (file and lines in each docstring), fed with the float32 inputs the kernel gets, widened.  The restatements
themselves are held against the reference's own functions run in float64 (tests/golden/reference_golden_geom_edges.npz, written
by tests/golden/generate_golden_geom_edges.py) by test_restatements_vs_reference_fp64, which needs no GPU.

Shapes: the tails and minimal sizes of every kernel's thread mapping (P = 1, P < 64, P % 64 != 0 for the one-wave kernels; P < 256,
P % 256 != 0 for the block_sum kernels; B = 1 / 63 / 64 / 65 / 257; ADD-S at the 2048-point chunk boundaries), the branches (z_min
clamp, portrait frames and crop sizes, centre outside the frame, im_id / obj_id given and null, n_sym null and n_sym < S, S = 1 and 64,
each term of the disentangled loss alone), objects of 5-30 cm at 0.3-2 m and a far, small one.

Real-valued results are judged PER ITEM (a batch maximum hides a small item behind a large one) and every case prints its measured
figure (-s).  Bounds are at most 3x the worst figure measured on an MI355X, and at most the ceilings of test_gpu_parity.py (GEOM_TOL
= 2e-6, DIST_TOL = 1e-5) unless the docstring derives why float32 cannot do better.  Index results are compared exactly: either on
inputs whose float64 costs are asserted, on the CPU, to be separated by a multiple of the float32 error bound, or on exact ties
(identical candidates), which pin the strict-<, first-wins rule.  u32 = 2^-24 is float32's unit roundoff throughout.
"""
import ctypes
import importlib.util
import pathlib

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

REPO = pathlib.Path(__file__).resolve().parent.parent
COSY_OK, COSY_EINVAL = 0, -1
U32 = 2.0 ** -24
Z_MIN, LAMB = float(np.float32(0.1)), float(np.float32(1.4))          # what the ABI's float arguments hold, widened
ADD_CHUNK = 2048                                                        # kernels_dist.hip: predicted points staged per pass


def _abi():
    from cosypose_amd._lib import lib, ptr, stream
    return lib(), ptr, stream


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to('cuda', dtype).contiguous()


def ints(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32)).to('cuda')


def host(t):
    return t.detach().cpu().numpy()


def report(tag, err, bound):
    print(f'  {tag}: {err:.3g} (bound {bound:g})')
    assert err < bound, (tag, err, bound)


def rows_err(got, want):
    """per item: max |got - want| / max |want| of that item -> (B,)"""
    a = np.asarray(got, np.float64).reshape(len(want), -1); b = np.asarray(want, np.float64).reshape(len(want), -1)
    return np.abs(a - b).max(axis=1) / np.maximum(np.abs(b).max(axis=1), 1e-300)


def pose_err(got, want):
    """per pose: rotation max |R - R'| (entries are O(1)); translation max |t - t'| / max |t'| of that pose -> two (B,)"""
    a = np.asarray(got, np.float64).reshape(-1, 4, 4); b = np.asarray(want, np.float64).reshape(-1, 4, 4)
    assert np.array_equal(a[:, 3], b[:, 3])                           # the last row is copied / constant: exact
    rot = np.abs(a[:, :3, :3] - b[:, :3, :3]).reshape(len(a), -1).max(axis=1)
    tn = np.abs(b[:, :3, 3]).max(axis=1)
    tr = np.abs(a[:, :3, 3] - b[:, :3, 3]).max(axis=1) / np.where(tn > 0, tn, 1.0)
    return rot, tr


# ---------------------------------------------------------------------------------------------------------------------------
# float64 restatements of the reference (numpy; `dt` = np.float32 evaluates the same lines in float32, for the findings)
# ---------------------------------------------------------------------------------------------------------------------------
def ref_transform_pts(T, pts):
    """lib3d/transform_ops.py:7-21: T (B,4,4) or (B,S,4,4), pts (B,P,3) -> (B,[S,]P,3) = R p + t"""
    if T.ndim == 4:
        pts = pts[:, None]
    return np.einsum('...ij,...pj->...pi', T[..., :3, :3], pts) + T[..., None, :3, 3]


def ref_project_points_robust(pts, K, TCO, z_min=Z_MIN):
    """camera_geometry.py:18-31: P = K @ TCO[:, :3]; suv = P [x y z 1]; the homogeneous z clamped to >= z_min; uv = suv.xy / z
    (torch.max propagates NaN, as np.maximum does)"""
    Pm = K @ TCO[:, :3]
    ph = np.concatenate([pts, np.ones(pts.shape[:2] + (1,), pts.dtype)], -1)
    suv = np.einsum('bij,bpj->bpi', Pm, ph)
    z = np.maximum(np.full_like(suv[..., 2], z_min), suv[..., 2])
    return suv[..., :2] / z[..., None]


def ref_boxes_from_uv(uv):
    """camera_geometry.py:34-42"""
    return np.stack([uv[..., 0].min(1), uv[..., 1].min(1), uv[..., 0].max(1), uv[..., 1].max(1)], 1)


def ref_deepim_boxes(center_uv, obs, rend, im_size, lamb=LAMB):
    """cropping.py:7-47 (clamp=False): a box of the frame's aspect around the projected centre that holds both boxes, times lamb"""
    xc, yc = center_uv[:, 0, 0], center_uv[:, 0, 1]
    r = max(im_size) / min(im_size)
    xdist = np.stack([np.abs(obs[:, 0] - xc), np.abs(rend[:, 0] - xc), np.abs(obs[:, 2] - xc), np.abs(rend[:, 2] - xc)], 1).max(1)
    ydist = np.stack([np.abs(obs[:, 1] - yc), np.abs(rend[:, 1] - yc), np.abs(obs[:, 3] - yc), np.abs(rend[:, 3] - yc)], 1).max(1)
    width = np.maximum(xdist, ydist * r) * 2 * lamb
    height = np.maximum(xdist / r, ydist) * 2 * lamb
    return np.stack([xc - width / 2, yc - height / 2, xc + width / 2, yc + height / 2], 1)


def ref_get_K_crop_resize(K, boxes, crop_resize):
    """camera_geometry.py:45-87: final_width = max(crop_resize), final_height = min(crop_resize) whatever their order"""
    fw, fh = max(crop_resize), min(crop_resize)
    cw, ch = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
    cj, ci = (boxes[:, 0] + boxes[:, 2]) / 2, (boxes[:, 1] + boxes[:, 3]) / 2
    cx = K[:, 0, 2] + (cw - 1) / 2 - cj
    cy = K[:, 1, 2] + (ch - 1) / 2 - ci
    dx, dy = cx - (cw - 1) / 2, cy - (ch - 1) / 2
    sx, sy = fw / cw, fh / ch
    out = K.copy()
    out[:, 0, 0] = sx * K[:, 0, 0]; out[:, 1, 1] = sy * K[:, 1, 1]
    out[:, 0, 2] = (fw - 1) / 2 + sx * dx; out[:, 1, 2] = (fh - 1) / 2 + sy * dy
    return out


def ref_crop_geometry(pts, K, TCO, im_size, crop, dt=np.float64):
    """PosePredictor.crop_inputs without the pixels (models/pose.py:45-67 with cropping.py:64-72: obs_boxes = rend_boxes)"""
    pts, K, TCO = (np.asarray(a, dt) for a in (pts, K, TCO))
    rend = ref_boxes_from_uv(ref_project_points_robust(pts, K, TCO, dt(Z_MIN)))
    center = ref_project_points_robust(np.zeros((len(pts), 1, 3), dt), K, TCO, dt(Z_MIN))
    crop_boxes = ref_deepim_boxes(center, rend, rend, im_size, dt(LAMB)).astype(dt)
    return rend, crop_boxes, ref_get_K_crop_resize(K, crop_boxes, crop).astype(dt), center


def ref_ortho6d(p6):
    """rotations.py:6-21: columns x, y, z"""
    x = p6[:, 0:3] / np.linalg.norm(p6[:, 0:3], axis=-1, keepdims=True)
    z = np.cross(x, p6[:, 3:6])
    z = z / np.linalg.norm(z, axis=-1, keepdims=True)
    return np.stack([x, np.cross(z, x), z], -1)


def ref_pose_update(TCO, K, pose9, dt=np.float64):
    """models/pose.py:69-79 (pose_dim 9) + cosypose_ops.py:10-31"""
    TCO, K, pose9 = (np.asarray(a, dt) for a in (TCO, K, pose9))
    out = TCO.copy()
    zsrc = TCO[:, 2, 3]
    ztgt = pose9[:, 8] * zsrc
    out[:, 2, 3] = ztgt
    out[:, 0, 3] = (pose9[:, 6] / K[:, 0, 0] + TCO[:, 0, 3] / zsrc) * ztgt
    out[:, 1, 3] = (pose9[:, 7] / K[:, 1, 1] + TCO[:, 1, 3] / zsrc) * ztgt
    out[:, :3, :3] = ref_ortho6d(pose9[:, :6]) @ TCO[:, :3, :3]
    return out


def ref_tco_init_from_boxes(z, boxes, K, dt=np.float64):
    """cosypose_ops.py:121-135 with z = mean(z_range)"""
    boxes, K = np.asarray(boxes, dt), np.asarray(K, dt)
    T = np.tile(np.eye(4, dtype=dt), (len(boxes), 1, 1))
    T[:, 0, 3] = ((boxes[:, 0] + boxes[:, 2]) / 2 - K[:, 0, 2]) * dt(z) / K[:, 0, 0]
    T[:, 1, 3] = ((boxes[:, 1] + boxes[:, 3]) / 2 - K[:, 1, 2]) * dt(z) / K[:, 1, 1]
    T[:, 2, 3] = z
    return T


def ref_tco_init_zup(boxes, pts, K, dt=np.float64):
    """cosypose_ops.py:138-173: z-up orientation at z = 1, depth from the extents of the model against those of the box"""
    boxes, pts, K = (np.asarray(a, dt) for a in (boxes, pts, K))
    T = np.tile(np.array([[0, 1, 0, 0], [0, 0, -1, 0], [-1, 0, 0, 1], [0, 0, 0, 1]], dt), (len(boxes), 1, 1))
    cu, cv = (boxes[:, 0] + boxes[:, 2]) / 2, (boxes[:, 1] + boxes[:, 3]) / 2
    T[:, 0, 3] = (cu - K[:, 0, 2]) * 1.0 / K[:, 0, 0]
    T[:, 1, 3] = (cv - K[:, 1, 2]) * 1.0 / K[:, 1, 1]
    C = ref_transform_pts(T, pts)
    dx3 = C[:, :, 0].max(1) - C[:, :, 0].min(1)
    dy3 = C[:, :, 1].max(1) - C[:, :, 1].min(1)
    z = (K[:, 1, 1] * dy3 / ((boxes[:, 3] - boxes[:, 1]) + 1) + K[:, 0, 0] * dx3 / ((boxes[:, 2] - boxes[:, 0]) + 1)) / 2
    T[:, 0, 3] = (cu - K[:, 0, 2]) * z / K[:, 0, 0]
    T[:, 1, 3] = (cv - K[:, 1, 2]) * z / K[:, 1, 1]
    T[:, 2, 3] = z
    return T, C


def ref_scatter_argmin(dists, ids, n_seg):
    """csrc/cosypose_cext.cpp:218-245: one pass; the first member of a segment seeds its minimum, a later one replaces it on
    strict <.  For a segment WITHOUT members the reference's output loop reads best_ids[n] of an unordered_map, which inserts and
    returns 0 (and lengthens the output by the inserted keys); the kernel's contract is -1 there, stated in cosyhip.h."""
    best, low = {}, {}
    for n, (v, e) in enumerate(zip(dists.tolist(), ids.tolist())):
        if e not in best:
            best[e], low[e] = n, v
        if v < low[e]:
            best[e], low[e] = n, v
    return np.array([best.get(s, -1) for s in range(n_seg)], np.int32)


def ref_expand_ids(n_sym_item):
    """csrc/cosypose_cext.cpp:247-259"""
    ids = [n for n, c in enumerate(n_sym_item) for _ in range(c)]
    syms = [k for c in n_sym_item for k in range(c)]
    return np.array(ids, np.int32), np.array(syms, np.int32)


def ref_sym_costs(T1, T2, pts, sym, dt=np.float64):
    """both cost tables of symmetric_distances.py over all S rows: (B,S) mean distance (mesh_points_dist :80-88, what
    symmetric_distance_batched :19-36 minimises over the first n_sym rows) and (B,S) mean SQUARED distance (:39-57)"""
    T1, T2, pts, sym = (np.asarray(a, dt) for a in (T1, T2, pts, sym))
    d = ref_transform_pts(T1[:, None] @ sym, pts) - ref_transform_pts(T2, pts)[:, None]
    sq = (d ** 2).sum(-1)
    return np.sqrt(sq).mean(-1), sq.mean(-1)


def first_min(costs, n):
    """index of the first minimum of costs[b, :n[b]] (strict <, first wins == np.argmin) -> (B,)"""
    return np.array([int(np.argmin(c[:k])) for c, k in zip(costs, n)], np.int32)


def ref_symmetric_distance(T1, T2, pts, sym, n_sym, mode, dt=np.float64):
    """mode 0: symmetric_distance_batched (:19-36) over the n_sym real rows; mode 1: ..._fast (:39-57) over the padded table.
    -> min_dists (B), best (B), S12 (B,4,4) and the cost table the choice was made on"""
    dist, sq = ref_sym_costs(T1, T2, pts, sym, dt)
    costs = dist if mode == 0 else sq
    best = first_min(costs, n_sym if mode == 0 else np.full(len(T1), sym.shape[1]))
    ar = np.arange(len(T1))
    return dist[ar, best], best, np.asarray(sym)[ar, best], costs


def ref_loss_co_costs(gt, pred, pts, dt=np.float64):
    """cosypose_ops.py:34-46 with l1: (B,S) mean over the 3P coordinates of |pred points - gt_s points|"""
    gt, pred, pts = (np.asarray(a, dt) for a in (gt, pred, pts))
    d = ref_transform_pts(pred, pts)[:, None] - ref_transform_pts(gt, pts)
    return np.abs(d).reshape(d.shape[0], d.shape[1], -1).mean(-1)


def ref_disentangled_preds(gt, Tin, out9, K, dt=np.float64):
    """cosypose_ops.py:49-82: the three predictions, each the first ground truth with one group of parameters replaced"""
    gt, Tin, out9, K = (np.asarray(a, dt) for a in (gt, Tin, out9, K))
    g0 = gt[:, 0]
    orn, xy, z = g0.copy(), g0.copy(), g0.copy()
    orn[:, :3, :3] = ref_ortho6d(out9[:, :6]) @ Tin[:, :3, :3]
    xy[:, 0, 3] = (out9[:, 6] / K[:, 0, 0] + Tin[:, 0, 3] / Tin[:, 2, 3]) * g0[:, 2, 3]
    xy[:, 1, 3] = (out9[:, 7] / K[:, 1, 1] + Tin[:, 1, 3] / Tin[:, 2, 3]) * g0[:, 2, 3]
    z[:, 2, 3] = out9[:, 8] * Tin[:, 2, 3]
    return orn, xy, z


def ref_disentangled(gt, Tin, out9, K, pts, dt=np.float64):
    """-> loss (B) = sum of the three terms' minima, and the three (B,S) cost tables"""
    tabs = [ref_loss_co_costs(gt, p, pts, dt) for p in ref_disentangled_preds(gt, Tin, out9, K, dt)]
    return sum(t.min(1) for t in tabs), tabs


def ref_dists_add(Tp, Tg, pts, dt=np.float64):
    """distances.py:5-9: gt points minus predicted points"""
    Tp, Tg, pts = (np.asarray(a, dt) for a in (Tp, Tg, pts))
    return ref_transform_pts(Tg, pts) - ref_transform_pts(Tp, pts)


def ref_dists_add_symmetric(Tp, Tg, pts, dt=np.float64, chunk=256):
    """distances.py:12-21: for every gt point j, gt_j minus the predicted point nearest to it (argmin over the predicted points of the
    squared distance: first minimum).  Also the nearest and second-nearest DISTANCES over the distinct predicted points (duplicated
    mesh points are one candidate: their residual is the same vector).  Walks the gt points in chunks: (P,P,3) does not fit at 4097."""
    Tp, Tg, pts = (np.asarray(a, dt) for a in (Tp, Tg, pts))
    pp, pg = ref_transform_pts(Tp, pts), ref_transform_pts(Tg, pts)
    B, P = pts.shape[:2]
    out, d1, d2 = np.empty((B, P, 3), dt), np.empty((B, P)), np.full((B, P), np.inf)
    for b in range(B):
        uniq = np.unique(np.asarray(pts[b]), axis=0, return_index=True)[1]
        for j0 in range(0, P, chunk):
            d = pg[b, None, j0:j0 + chunk] - pp[b, :, None]                      # (P pred, chunk gt, 3)
            sq = (d ** 2).sum(-1)
            a = sq.argmin(0)
            cols = np.arange(sq.shape[1])
            out[b, j0:j0 + chunk] = d[a, cols]
            d1[b, j0:j0 + chunk] = np.sqrt(sq[a, cols])
            if len(uniq) > 1:
                d2[b, j0:j0 + chunk] = np.sqrt(np.partition(sq[uniq], 1, axis=0)[1])
    return out, d1, d2


# ---------------------------------------------------------------------------------------------------------------------------
# seeded inputs
# ---------------------------------------------------------------------------------------------------------------------------
def rand_rot(rs):
    q, r = np.linalg.qr(rs.randn(3, 3))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def rand_poses(rs, n, z=(0.3, 2.0), xy=0.2):
    """rigid poses, float32: the object 0.3-2 m in front of the camera, inside a +-0.2 z wide cone"""
    T = np.tile(np.eye(4), (n, 1, 1))
    for i in range(n):
        T[i, :3, :3] = rand_rot(rs)
        zz = rs.uniform(*z)
        T[i, :3, 3] = (rs.uniform(-xy, xy) * zz, rs.uniform(-xy, xy) * zz, zz)
    return T.astype(np.float32)


def rand_K(rs, n, h, w):
    """fx != fy, principal point off centre"""
    K = np.tile(np.eye(3, dtype=np.float32), (n, 1, 1))
    K[:, 0, 0] = rs.uniform(0.8, 1.4, n) * max(h, w); K[:, 1, 1] = K[:, 0, 0] * rs.uniform(0.9, 1.1, n)
    K[:, 0, 2] = w / 2 + rs.uniform(-15, 15, n); K[:, 1, 2] = h / 2 + rs.uniform(-15, 15, n)
    return K


def rand_mesh(rs, n_obj, P, ext=(0.05, 0.3)):
    """n_obj point sets of P points in boxes of 5-30 cm per axis, float32"""
    return (rs.uniform(-1, 1, (n_obj, P, 3)) * rs.uniform(ext[0] / 2, ext[1] / 2, (n_obj, 1, 3))).astype(np.float32)


def rand_boxes(rs, n, h, w):
    """detections of different aspect, partly outside the frame"""
    cx, cy = rs.uniform(0, w, n), rs.uniform(0, h, n)
    bw, bh = rs.uniform(8, 0.6 * w, n), rs.uniform(8, 0.6 * h, n)
    return np.stack([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], 1).astype(np.float32)


def sym_table(rs, n_obj, S, n_sym):
    """identity-padded (n_obj,S,4,4): row k < n_sym = rotation by 2 pi k / n_sym about z plus a millimetre offset"""
    sym = np.tile(np.eye(4, dtype=np.float32), (n_obj, S, 1, 1))
    for o in range(n_obj):
        for k in range(1, n_sym[o]):
            a = 2 * np.pi * k / n_sym[o]
            sym[o, k, :3, :3] = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], np.float32)
            sym[o, k, :3, 3] = (rs.randn(3) * 0.002).astype(np.float32)
    return sym


def small_motion(rs, rot=0.02, trans=0.003):
    m = np.eye(4); m[:3, :3] += rot * rs.randn(3, 3); m[:3, 3] = rs.randn(3) * trans
    return m


# ---------------------------------------------------------------------------------------------------------------------------
# separation of index results: asserted on the CPU, from float64 alone, before any kernel runs
# ---------------------------------------------------------------------------------------------------------------------------
SEP_MULT = 8          # margin = SEP_MULT x the float32 error bound of the compared cost


def point_cost_err_bound(*Ts):
    """float32 error bound of a mean over points of a distance (or of |coordinate differences|) between two transformed point
    sets: each transformed coordinate is 3 products and 3 sums of magnitude <= Z = max |entry of the result| -> 6 u32 Z per
    coordinate, two sets, three coordinates of a norm (<= sqrt 3 x), a product of two 4x4 matrices in front (4 more), plus the
    mean's own roundings, which are relative to the cost <= Z: 32 u32 Z in all, per item.  Z is taken as |t| + the mesh radius."""
    Z = np.maximum.reduce([np.abs(np.asarray(T, np.float64)[..., :3, 3]).max(axis=tuple(range(1, np.asarray(T).ndim - 1))) for T in Ts])
    return 32 * U32 * (Z + 0.3)


def assert_separated(costs, n, err_bound, same=None):
    """every item's float64 minimum beats every other candidate by > SEP_MULT x err_bound[b] -- except candidates that are the SAME
    input bit for bit (same[b, s] = first row identical to row s), whose costs are equal in any precision: those are exact ties,
    and the expected index is the first of them."""
    for b, (c, k) in enumerate(zip(costs, n)):
        c = c[:k]
        i = int(np.argmin(c))
        for s in range(k):
            if s == i or (same is not None and same[b][s] == same[b][i]):
                assert c[s] == c[i]
                continue
            assert c[s] - c[i] > SEP_MULT * err_bound[b], (b, s, i, c[s] - c[i], SEP_MULT * err_bound[b])


def first_identical(rows):
    """rows (B,S,...) -> (B,S) index of the first row of the item that is bitwise equal to row s"""
    B, S = rows.shape[:2]
    out = np.zeros((B, S), int)
    for b in range(B):
        for s in range(S):
            out[b, s] = next(k for k in range(s + 1) if np.array_equal(rows[b, k], rows[b, s]))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# cases (built on the CPU; the non-GPU test below checks every precondition)
# ---------------------------------------------------------------------------------------------------------------------------
def crop_case(name):
    """-> dict(table, obj, K, im, TCO, im_size, crop): object table (n_obj,P,3), obj (B), K (N,3,3) with im (B) or (B,3,3) with None"""
    B, P, im_size, crop, flavour = CROP_CASES[name]
    rs = np.random.RandomState(sum(map(ord, name)))
    n_obj = min(B, 5)
    table = rand_mesh(rs, n_obj, P)
    obj = rs.randint(0, n_obj, B).astype(np.int32)
    h, w = im_size
    TCO = rand_poses(rs, B)
    K, im = rand_K(rs, B, h, w), None
    if flavour == 'imid':
        K = rand_K(rs, 5, h, w); im = rs.randint(0, 5, B).astype(np.int32); im[:5] = np.arange(5)
    if flavour == 'behind':                                  # the clamp: items with points behind z_min, one with points exactly on it
        for b in range(0, B, 2):
            TCO[b, :3, 3] = (rs.uniform(-0.02, 0.02), rs.uniform(-0.02, 0.02), rs.uniform(0.02, 0.15))
        TCO[1, :3, :3] = np.eye(3); TCO[1, :3, 3] = (0.03, 0.02, np.float32(0.1))
        table[obj[1], 0] = 0.0; table[obj[1], P // 2] = (0.01, -0.02, 0.0)
    if flavour == 'outside':                                 # the object's centre projects outside the frame
        for b in range(B):
            TCO[b, :2, 3] = np.array([rs.choice([-1, 1]) * rs.uniform(0.7, 1.2), rs.choice([-1, 1]) * rs.uniform(0.6, 0.9)]) * TCO[b, 2, 3]
    if flavour == 'far':                                     # 3-6 cm objects at 4-8 m: boxes of a few pixels
        table = rand_mesh(rs, n_obj, P, ext=(0.03, 0.06)); TCO = rand_poses(rs, B, z=(4.0, 8.0))
    return dict(table=table, obj=obj, K=K, im=im, TCO=TCO, im_size=im_size, crop=crop)


CROP_CASES = {
    # name: (B, P, frame (h, w), crop size (h, w), flavour)
    'plain': (6, 2000, (480, 640), (240, 320), ''),
    'square_crop': (6, 300, (480, 640), (256, 256), ''),
    'P1': (4, 1, (480, 640), (240, 320), ''),
    'P2': (4, 2, (480, 640), (240, 320), ''),
    'P63': (3, 63, (480, 640), (240, 320), ''),
    'P64': (3, 64, (480, 640), (240, 320), ''),
    'P65': (3, 65, (480, 640), (240, 320), ''),
    'P130': (2, 130, (480, 640), (240, 320), ''),
    'B1': (1, 500, (480, 640), (240, 320), ''),
    'B257': (257, 200, (480, 640), (240, 320), ''),
    'portrait_frame': (6, 500, (640, 480), (240, 320), ''),
    'portrait_crop': (6, 500, (480, 640), (320, 240), ''),
    'portrait_both': (6, 500, (640, 480), (320, 240), ''),
    'behind': (8, 70, (480, 640), (240, 320), 'behind'),
    'outside': (8, 500, (480, 640), (240, 320), 'outside'),
    'imid': (37, 100, (480, 640), (240, 320), 'imid'),
    'far': (16, 500, (480, 640), (240, 320), 'far'),
}


def sd_case(name):
    """symmetric distance: -> dict(table, sym, n_sym, obj, T1, T2) with T1 = T2 . sym_k^-1 . small motion (k = 0 often: the
    identity-padded rows then tie with row 0 exactly)"""
    B, P, S, nmax, flavour = SD_CASES[name]
    rs = np.random.RandomState(sum(map(ord, name)) + 1000)
    n_obj = B if flavour == 'rows' else min(B, 4)
    n_sym = rs.randint(1, nmax + 1, n_obj).astype(np.int32)
    n_sym[0] = nmax
    table = rand_mesh(rs, n_obj, P, ext=(0.06, 0.3))
    table[:, :, 0] *= 1.5                                    # no accidental symmetry about z
    sym = sym_table(rs, n_obj, S, n_sym)
    if flavour == 'junk':                                    # rows past n_sym are NOT identity: mode 0 must not look at them
        for o in range(n_obj):
            for k in range(n_sym[o], S):
                sym[o, k, :3, :3] = rand_rot(rs); sym[o, k, :3, 3] = rs.randn(3) * 0.002
    obj = np.arange(B, dtype=np.int32) if flavour == 'rows' else rs.randint(0, n_obj, B).astype(np.int32)
    T2 = rand_poses(rs, B, z=(4.0, 8.0) if flavour == 'far' else (0.3, 2.0))
    T1 = T2.copy()
    for b in range(B):
        k = rs.randint(0, S if flavour == 'junk' else n_sym[obj[b]]) if b % 3 else 0
        T1[b] = (T2[b].astype(np.float64) @ np.linalg.inv(sym[obj[b], k].astype(np.float64))
                 @ small_motion(rs, trans=0.0003 if flavour == 'far' else 10 ** rs.uniform(-3.5, -1.5))).astype(np.float32)
    return dict(table=table, sym=sym, n_sym=n_sym, obj=obj, T1=T1, T2=T2, rows=flavour == 'rows')


SD_CASES = {
    # name: (B, P, S, largest n_sym, flavour)      'rows': obj_id null, item b uses table row b
    'P1': (5, 1, 4, 1, ''),                        # one point: every rotation about it costs the same offset -> n_sym = 1
    'P63': (5, 63, 4, 4, ''),
    'P255': (5, 255, 4, 4, ''),
    'P256': (5, 256, 4, 4, ''),
    'P257': (5, 257, 4, 4, ''),
    'P2000': (9, 2000, 8, 8, ''),
    'S1': (9, 300, 1, 1, ''),
    'S64': (5, 100, 64, 64, ''),
    'padded': (9, 300, 8, 3, ''),                  # n_sym <= 3 < S = 8: five identity rows at least
    'B1': (1, 300, 4, 4, ''),
    'B257': (257, 70, 4, 4, ''),
    'rows': (9, 300, 4, 4, 'rows'),
    'junk_padding': (12, 300, 8, 3, 'junk'),       # T1 often matches a row past n_sym: mode 1 takes it, mode 0 must not
    'far': (9, 500, 4, 4, 'far'),
}


def sd_expect(c, mode, use_nsym=True):
    """float64 expectation of one mode + the separation precondition"""
    pts = c['table'][c['obj']]
    sym = c['sym'][c['obj']]
    n = c['n_sym'][c['obj']] if (mode == 0 and use_nsym) else np.full(len(pts), sym.shape[1], np.int32)
    d, best, S12, costs = ref_symmetric_distance(c['T1'], c['T2'], pts, sym, n, mode)
    eb = point_cost_err_bound(c['T1'], c['T2'])
    if mode == 1:
        eb = eb * 2 * np.sqrt(np.maximum(costs.max(1), 1e-30))          # a squared distance: d(x^2) = 2 x dx
    assert_separated(costs, n, eb, first_identical(sym))
    return d, best, S12


def loss_case(name):
    """losses: -> dict(table, obj, gt (B,S,4,4), pred, Tin, out9, K).  Ground truths T . sym_k over an identity-padded table and,
    for flavour 'dup', row 2 a copy of row 0 (exact ties); pred = gt_k . small motion"""
    B, P, S, flavour = LOSS_CASES[name]
    rs = np.random.RandomState(sum(map(ord, name)) + 2000)
    n_obj = min(B, 4)
    n_sym = np.minimum(rs.randint(1, 5, n_obj), S).astype(np.int32)
    table = rand_mesh(rs, n_obj, P, ext=(0.06, 0.3)); table[:, :, 0] *= 1.5
    sym = sym_table(rs, n_obj, S, n_sym)
    obj = rs.randint(0, n_obj, B).astype(np.int32)
    T = rand_poses(rs, B, z=(4.0, 8.0) if flavour == 'far' else (0.3, 2.0))
    gt = (T[:, None].astype(np.float64) @ sym[obj].astype(np.float64)).astype(np.float32)
    if flavour == 'dup' and S > 2:
        gt[:, 2] = gt[:, 0]
    pred = np.stack([(gt[b, rs.randint(0, n_sym[obj[b]]) if b % 3 else 0].astype(np.float64)
                      @ small_motion(rs, trans=10 ** rs.uniform(-3.5, -1.5))) for b in range(B)]).astype(np.float32)
    # disentangled loss: the input pose is the prediction; outputs near the identity update; K_crop with fx != fy
    out9 = (rs.randn(B, 9) * 0.05 + np.array([1, 0, 0, 0, 1, 0, 0, 0, 1])).astype(np.float32)
    out9[:, 6:8] = rs.randn(B, 2) * 3                                     # a few pixels
    K = np.tile(np.eye(3, dtype=np.float32), (B, 1, 1))
    K[:, 0, 0] = rs.uniform(900, 2500, B); K[:, 1, 1] = K[:, 0, 0] * rs.uniform(0.7, 1.3, B); K[:, 0, 2] = 160; K[:, 1, 2] = 120
    return dict(table=table, obj=obj, gt=gt, pred=pred, Tin=pred.copy(), out9=out9, K=K)


LOSS_CASES = {
    # name: (B, P, S, flavour)
    'P1': (5, 1, 1, ''),
    'P255': (5, 255, 4, ''),
    'P256': (5, 256, 4, ''),
    'P257': (5, 257, 4, 'dup'),
    'P2000': (9, 2000, 4, 'dup'),
    'S1': (9, 300, 1, ''),
    'S8': (9, 300, 8, 'dup'),
    'B1': (1, 300, 4, ''),
    'B257': (257, 70, 4, 'dup'),
    'far': (9, 500, 4, 'far'),
}


def loss_expect(c):
    pts = c['table'][c['obj']]
    costs = ref_loss_co_costs(c['gt'], c['pred'], pts)
    S = costs.shape[1]
    assert_separated(costs, np.full(len(costs), S), point_cost_err_bound(c['gt'], c['pred'][:, None]), first_identical(c['gt']))
    return costs.min(1), costs.argmin(1).astype(np.int32)


def disentangled_per_term_case():
    """S = 3 ground truths built so that the three terms are assigned DIFFERENT ones: gt 0 anchors the predictions; gt 1 has the
    orientation the update predicts (and a 1 cm offset), so the orientation term prefers it; gt 2 has gt 0's orientation and the depth
    the update predicts, so the depth term prefers it; the xy term stays with gt 0."""
    rs = np.random.RandomState(4242)
    B, P = 9, 300
    table = rand_mesh(rs, B, P, ext=(0.1, 0.3))
    Tin = rand_poses(rs, B)
    out9 = (rs.randn(B, 9) * 0.02 + np.array([1, 0, 0, 0, 1, 0, 0, 0, 1])).astype(np.float32)
    out9[:, :6] = (np.array([1, 0, 0, 0, 1, 0]) + rs.randn(B, 6) * 0.5).astype(np.float32)       # a large rotation update
    out9[:, 6:8] = rs.randn(B, 2).astype(np.float32)
    out9[:, 8] = rs.choice([0.7, 1.4], B)
    K = np.tile(np.array([[1200., 0, 160], [0, 1000., 120], [0, 0, 1]], np.float32), (B, 1, 1))
    g0 = Tin.copy()
    g0[:, :3, 3] += (rs.randn(B, 3) * 0.002).astype(np.float32)
    orn, _, z = ref_disentangled_preds(g0[:, None], Tin, out9, K)
    g1 = orn.copy(); g1[:, :3, 3] += 0.01
    g2 = z.copy(); g2[:, :3, 3] += 0.002
    gt = np.stack([g0, g1.astype(np.float32), g2.astype(np.float32)], 1)
    return dict(table=table, obj=np.arange(B, dtype=np.int32), gt=gt, Tin=Tin, out9=out9, K=K)


ADDS_CASES = {
    # name: (B, P, duplicated points)       P = 2048 / 2049 / 4097: the ADD_CHUNK boundaries
    'P1': (2, 1, 0), 'P100': (3, 100, 10), 'P255': (2, 255, 0), 'P257': (2, 257, 0), 'P2048': (2, 2048, 100), 'P2049': (2, 2049, 0),
    'P4097': (2, 4097, 100),
}
ADDS_SEP_MULT = 4                                    # nearest vs second-nearest DISTANCE: margin = 4 x the bound of one distance
ADDS_MAX_EXCLUDED = 0.01


def adds_case(name):
    B, P, dup = ADDS_CASES[name]
    rs = np.random.RandomState(sum(map(ord, name)) + 3000)
    pts = rand_mesh(rs, B, P, ext=(0.1, 0.3))
    if dup:
        pts[:, P // 2:P // 2 + dup] = pts[:, :dup]
    Tg = rand_poses(rs, B)
    Tp = np.stack([Tg[b].astype(np.float64) @ small_motion(rs, rot=0.1, trans=0.01) for b in range(B)]).astype(np.float32)
    return dict(pts=pts, Tp=Tp, Tg=Tg)


def adds_expect(c):
    """float64 residuals, and the points whose nearest predicted point is separated from the runner-up"""
    want, d1, d2 = ref_dists_add_symmetric(c['Tp'], c['Tg'], c['pts'])
    eb = point_cost_err_bound(c['Tp'], c['Tg'])[:, None]
    sep = (d2 - d1) > ADDS_SEP_MULT * eb
    return want, sep, eb


# ---------------------------------------------------------------------------------------------------------------------------
# non-GPU: the restatements against the reference in float64, and every seeded case's preconditions
# ---------------------------------------------------------------------------------------------------------------------------
def _edge_module():
    spec = importlib.util.spec_from_file_location('generate_golden_geom_edges', REPO / 'tests' / 'golden' / 'generate_golden_geom_edges.py')
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


FP64_TOL = 1e-13          # float64 rounding over a few dozen operations, relative per item (measured worst 1.6e-14)


def test_restatements_vs_reference_fp64():
    """Every restatement above against the reference's own function evaluated in float64 on the same inputs
    (reference_golden_geom_edges.npz): crop geometry at portrait frame + portrait crop, landscape, landscape frame + portrait crop,
    with points behind and exactly on the z_min clamp and a centre outside the frame; pose update; both initialisations; symmetric
    distance in both modes with n_sym < S; loss_CO_symmetric and the disentangled loss with S = 4 ground truths; ADD and ADD-S.
    Chosen symmetries and assigned ground truths are compared exactly."""
    m = _edge_module()
    d = m.edge_inputs()
    g = dict(np.load(m.OUT, allow_pickle=False))
    worst = 0.0

    def close(tag, got, want):
        nonlocal worst
        e = float(rows_err(got, want).max())
        worst = max(worst, e)
        print(f'  {tag}: {e:.3g}')
        assert e < FP64_TOL, (tag, e)

    for tag, im_size, crop in (('pp', (640, 480), (320, 240)), ('ll', (480, 640), (240, 320)), ('lp', (480, 640), (320, 240))):
        rend, cb, kc, _ = ref_crop_geometry(d['cg_pts'], d['cg_K'], d['cg_TCO'], im_size, crop)
        close(f'crop {tag} boxes_rend', rend, g[f'cg_{tag}_boxes_rend'])
        close(f'crop {tag} boxes_crop', cb, g[f'cg_{tag}_boxes_crop'])
        close(f'crop {tag} K_crop', kc, g[f'cg_{tag}_K_crop'])
    assert np.array_equal(g['cg_ll_K_crop'], g['cg_lp_K_crop'])      # the reference sorts the crop size: (240, 320) == (320, 240)
    close('pose_update', ref_pose_update(d['cg_TCO'], g['cg_ll_K_crop'], d['pu_pose9']), g['pu_TCO_out'])
    close('init_from_boxes', ref_tco_init_from_boxes(1.0, d['init_boxes'], d['cg_K']), g['init_v0'])
    close('init_zup', ref_tco_init_zup(d['init_boxes'], d['cg_pts'], d['cg_K'])[0], g['init_zup'])
    pts, sym, n = d['sd_pts'][d['sd_obj']], d['sd_sym'][d['sd_obj']], d['sd_nsym'][d['sd_obj']]
    for mode, name in ((0, 'batched'), (1, 'fast')):
        dist, best, S12, _ = ref_symmetric_distance(d['sd_T1'], d['sd_T2'], pts, sym, n, mode)
        close(f'symmetric_distance {name}', dist, g[f'sd_{name}_dists'])
        assert np.array_equal(S12.astype(np.float64), g[f'sd_{name}_S12'])
        assert len(set(best.tolist())) > 1                                          # a non-trivial choice
    gt = (d['sd_T2'][:, None].astype(np.float64) @ sym.astype(np.float64))
    costs = ref_loss_co_costs(gt, d['sd_T1'], pts)
    close('loss_CO_symmetric', costs.min(1), g['ls_loss'])
    assert np.array_equal(gt[np.arange(len(gt)), costs.argmin(1)], g['ls_assign'])
    close('loss_refiner_CO_disentangled', ref_disentangled(gt, d['sd_T1'], d['ls_out9'], d['ls_K_crop'], pts)[0], g['ls_disentangled'])
    close('dists_add', ref_dists_add(d['sd_T1'], d['sd_T2'], pts), g['add'])
    close('dists_add_symmetric', ref_dists_add_symmetric(d['sd_T1'], d['sd_T2'], pts)[0], g['adds'])
    print(f'  worst: {worst:.3g}')


def test_index_case_preconditions():
    """From float64 alone: every symmetric-distance and loss case is separated by SEP_MULT x its float32 error bound (exact ties
    apart), the per-term case assigns three different ground truths, and every ADD-S case excludes at most 1 % of its points from
    the vector comparison."""
    for name in SD_CASES:
        c = sd_case(name)
        for mode in (0, 1):
            _, best, _ = sd_expect(c, mode)
        if name in ('padded', 'P2000'):
            sd_expect(c, 0, use_nsym=False)
    for name in LOSS_CASES:
        loss_expect(loss_case(name))
    c = disentangled_per_term_case()
    _, tabs = ref_disentangled(c['gt'], c['Tin'], c['out9'], c['K'], c['table'][c['obj']])
    eb = point_cost_err_bound(c['gt'], c['Tin'][:, None])
    for t in tabs:
        assert_separated(t, np.full(len(t), 3), eb)
    assign = np.stack([t.argmin(1) for t in tabs], 1)
    assert np.array_equal(assign, np.tile([1, 0, 2], (len(assign), 1))), assign
    for name in ADDS_CASES:
        _, sep, _ = adds_expect(adds_case(name))
        excluded = int((~sep).sum(axis=1).max())
        print(f'  ADD-S {name}: {excluded} of {sep.shape[1]} points excluded')
        assert excluded <= ADDS_MAX_EXCLUDED * sep.shape[1], (name, excluded)


# ---------------------------------------------------------------------------------------------------------------------------
# crop geometry
# ---------------------------------------------------------------------------------------------------------------------------
BOX_TOL = 8e-7            # boxes_rend / boxes_crop, per item relative to the item's largest coordinate (measured worst 2.7e-7, case 'outside')
K_CROP_TOL = 2e-6         # K_crop likewise: GEOM_TOL itself (measured worst 1.84e-6 at P = 1, 1.5e-6 at P = 2 and B = 257; median 6e-7)
FAR_C = 5.0               # K_crop of the far, small object in the unit derived in test_crop_geometry_vs_fp64 (measured 1.98; float32 numpy 1.81)


def run_crop_geometry(c):
    lib, ptr, stream = _abi()
    B, P = len(c['TCO']), c['table'].shape[1]
    t, o, K, im, T = dev(c['table']), ints(c['obj']), dev(c['K']), ints(c['im']), dev(c['TCO'])
    br, bc, kc = (torch.full((B, n), 7.0, device='cuda') for n in (4, 4, 9))
    rc = lib.cosy_crop_geometry(ptr(t), ptr(o), ptr(K), ptr(im), ptr(T), B, P, Z_MIN, c['im_size'][0], c['im_size'][1], c['crop'][0],
                                c['crop'][1], LAMB, ptr(br), ptr(bc), ptr(kc), stream())
    assert rc == COSY_OK, lib.cosy_last_error()
    return br, bc, kc.view(B, 3, 3)


def crop_expect(c, dt=np.float64):
    K = c['K'] if c['im'] is None else c['K'][c['im']]
    return ref_crop_geometry(c['table'][c['obj']], K, c['TCO'], c['im_size'], c['crop'], dt)


@gpu
@pytest.mark.parametrize('name', list(CROP_CASES))
def test_crop_geometry_vs_fp64(name):
    """cosy_crop_geometry against crop_inputs' geometry in float64: P = 1 .. 2000 around the 64-lane tails, B = 1 .. 257, portrait
    frames (r = max / min of the frame) and portrait crop sizes (final_width = max of the crop size), points behind and exactly on
    the z_min clamp, centres outside the frame, K per frame through im_id over 5 frames, shuffled object ids.

    boxes_rend, boxes_crop: per item relative to the item's largest coordinate.  K_crop the same, except case 'far'.
    Derivation for 'far' (3-6 cm at 4-8 m: a box of ~10 pixels, hundreds of pixels from the origin): a projected coordinate
    carries ~12 roundings (3 for its row of K @ TCO, 4 + 4 for the two dot products, 1 division): 12 u32 M with M the item's
    largest |coordinate|.  The box half-size |x - xc| subtracts two such numbers and the corners xc -+ width / 2 and their
    difference add 4 more roundings at magnitude M, so the crop's width cw is off by <= 32 u32 M, i.e. relatively by
    32 u32 M / (cw / (2 lamb)) against the un-inflated extent.  K_crop's focal lengths are fw / cw times K's and its principal point
    is scale x (K's minus the box centre), so the item's error relative to its largest entry is <= FAR_C u32 A g with
    A = 2 lamb M / min(cw, ch) and g = max(1, |cx - cj| / fx, |cy - ci| / fy), with FAR_C <= 32 by this count.  No float32
    evaluation of the reference's formula avoids it: the same lines in numpy float32 are printed beside the kernel and land at the
    same level (raw error 1.13e-5 against the kernel's 1.24e-5 at A = 60 .. 137; 1.81 against 1.98 in the derived unit), so the
    kernel is left as it is and the bound is 5 units, well inside the 32 of the count.
    Measured worst on an MI355X: boxes_rend 1.63e-7, boxes_crop 2.7e-7 (bound 8e-7); K_crop 1.84e-6 (P = 1: one point, a box as small
    as the point is close to the centre; bound 2e-6 = GEOM_TOL); far K_crop 1.98 units (bound 5)."""
    c = crop_case(name)
    rend, cb, kc, center = crop_expect(c)
    br, bc, kk = run_crop_geometry(c)
    report(f'{name} boxes_rend', float(rows_err(host(br), rend).max()), BOX_TOL)
    report(f'{name} boxes_crop', float(rows_err(host(bc), cb).max()), BOX_TOL)
    e = rows_err(host(kk), kc)
    if name != 'far':
        report(f'{name} K_crop', float(e.max()), K_CROP_TOL)
    else:
        K = c['K'] if c['im'] is None else c['K'][c['im']]
        M = np.maximum(np.abs(rend).max(1), np.abs(center[:, 0]).max(1))
        cw, ch = cb[:, 2] - cb[:, 0], cb[:, 3] - cb[:, 1]
        A = 2 * LAMB * M / np.minimum(cw, ch)
        g = np.maximum(1.0, np.maximum(np.abs(K[:, 0, 2] - (cb[:, 0] + cb[:, 2]) / 2) / K[:, 0, 0], np.abs(K[:, 1, 2] - (cb[:, 1] + cb[:, 3]) / 2) / K[:, 1, 1]))
        e32 = rows_err(crop_expect(c, np.float32)[2], kc)
        print(f'  far: amplification A = {A.min():.3g} .. {A.max():.3g}; K_crop raw error {e.max():.3g}, float32 numpy {e32.max():.3g}')
        print(f'  far: float32 numpy in the derived unit: {float((e32 / (U32 * A * g)).max()):.3g}')
        report('far K_crop / (u32 A g)', float((e / (U32 * A * g)).max()), FAR_C)
    # the three outputs are complete and deterministic
    br2, bc2, kk2 = run_crop_geometry(c)
    assert torch.equal(br, br2) and torch.equal(bc, bc2) and torch.equal(kk, kk2)


@gpu
def test_crop_geometry_nan_item_leaves_the_others_alone():
    """A NaN translation and NaN rotation entries in three of 37 items (K through im_id): those items' boxes are NaN, as the
    reference's min / max give them (the restatement agrees), and every other item is bit-identical to the run without them."""
    c = crop_case('imid')
    clean = run_crop_geometry(c)
    bad = [3, 17, 30]
    c['TCO'] = c['TCO'].copy()
    c['TCO'][3, 0, 3] = np.nan; c['TCO'][17, 1, 1] = np.nan; c['TCO'][30, 2, 2] = np.nan
    got = run_crop_geometry(c)
    keep = torch.tensor([b for b in range(len(c['obj'])) if b not in bad], device='cuda')
    for a, b in zip(got, clean):
        assert torch.equal(a[keep], b[keep])
    with np.errstate(invalid='ignore'):
        rend, cb, _, _ = crop_expect(c)
    assert np.isnan(rend[bad]).any(1).all() and np.isnan(cb[bad]).all()
    assert all(bool(torch.isnan(got[0][b]).any()) and bool(torch.isnan(got[1][b]).all()) for b in bad)


# ---------------------------------------------------------------------------------------------------------------------------
# pose update and the two initialisations
# ---------------------------------------------------------------------------------------------------------------------------
POSE_ROT_TOL = 4.5e-7     # rotation entries, absolute per pose (measured worst 1.62e-7, pose update at B = 65)
POSE_TR_TOL = 2e-7        # translation relative to the pose's own largest entry (measured worst 5.9e-8 pose update, 7.6e-8 init from boxes)
BATCH_SIZES = [1, 63, 64, 65, 257]


@gpu
@pytest.mark.parametrize('B', BATCH_SIZES)
def test_pose_update_vs_fp64(B):
    """cosy_pose_update at B around the 64-thread workgroup, K_crop with fx != fy (a swapped fx / fy moves the translation by 10-30 %),
    update vectors near the identity as a network gives them.  Rotation and translation per pose.
    Measured worst: rotation 1.62e-7 (bound 4.5e-7), translation 5.9e-8 (bound 2e-7)."""
    lib, ptr, stream = _abi()
    rs = np.random.RandomState(100 + B)
    TCO = rand_poses(rs, B)
    K = rand_K(rs, B, 240, 320); K[:, 0, 0] *= 3; K[:, 1, 1] *= rs.uniform(2.0, 4.0, B).astype(np.float32)
    pose9 = (rs.randn(B, 9) * 0.2 + np.array([1, 0, 0, 0, 1, 0, 0, 0, 1])).astype(np.float32)
    pose9[:, 6:8] = rs.randn(B, 2) * 20
    out = torch.full((B + 1, 4, 4), 7.0, device='cuda')                      # one spare row: the b >= B guard
    T, Kd, pd = dev(TCO), dev(K), dev(pose9)
    assert lib.cosy_pose_update(ptr(T), ptr(Kd), ptr(pd), B, ptr(out), stream()) == COSY_OK
    assert bool((out[B] == 7.0).all())
    rot, tr = pose_err(host(out[:B]), ref_pose_update(TCO, K, pose9))
    report(f'B={B} rotation', float(rot.max()), POSE_ROT_TOL)
    report(f'B={B} translation', float(tr.max()), POSE_TR_TOL)


@gpu
@pytest.mark.parametrize('B', BATCH_SIZES)
@pytest.mark.parametrize('with_im', [False, True])
def test_tco_init_from_boxes_vs_fp64(B, with_im):
    """cosy_tco_init_from_boxes: boxes of different aspect, partly outside the frame, fx != fy, K per item or per frame (3 frames).
    Measured worst: 7.6e-8 (bound 2e-7); the rotation is the identity, exactly."""
    lib, ptr, stream = _abi()
    rs = np.random.RandomState(200 + B)
    boxes = rand_boxes(rs, B, 480, 640)
    K = rand_K(rs, 3 if with_im else B, 480, 640)
    im = rs.randint(0, 3, B).astype(np.int32) if with_im else None
    z = float(np.float32(np.mean(np.float32([0.75, 1.35]))))
    out = torch.full((B + 1, 4, 4), 7.0, device='cuda')
    b_, K_, im_ = dev(boxes), dev(K), ints(im)
    assert lib.cosy_tco_init_from_boxes(ptr(b_), ptr(K_), ptr(im_), B, z, ptr(out), stream()) == COSY_OK
    assert bool((out[B] == 7.0).all())
    rot, tr = pose_err(host(out[:B]), ref_tco_init_from_boxes(z, boxes, K if im is None else K[im]))
    assert rot.max() == 0.0
    report(f'B={B} im_id={int(with_im)} translation', float(tr.max()), POSE_TR_TOL)


ZUP_C = 3.0               # in the unit derived in test_tco_init_zup_autodepth_vs_fp64 (measured worst 1.12; float32 numpy 1.12)
ZUP_CASES = [(4, 1, False), (4, 2, True), (3, 63, False), (3, 64, True), (3, 65, False), (2, 130, True), (6, 2000, False), (1, 500, True),
             (257, 100, True)]


@gpu
@pytest.mark.parametrize('B,P,with_im', ZUP_CASES)
def test_tco_init_zup_autodepth_vs_fp64(B, P, with_im):
    """cosy_tco_init_zup_autodepth at P = 1 .. 2000 around the 64-lane tails, B = 1 .. 257, im_id given and null, shuffled object ids.
    P = 1: the model has no extent, depth 0, and the kernel's pose equals the reference's exactly.
    Derivation of the bound: the depth is f x (max - min of a camera coordinate) / (box size), and the camera coordinates are model
    coordinates PLUS the z = 1 translation (up to ~0.6), one rounding each: the extent max - min of a 5-30 cm model carries
    2 u32 |c| / extent relative error -- 10 u32 for a 10 cm model at the frame's edge, more than GEOM_TOL for a two-point model of a
    few centimetres.  The reference's float32 does the same subtraction.  With 6 more roundings for the products, quotients and the
    mean, a pose's translation is off by <= 8 u32 (1 + a) relative, a = max over x, y of max |c| / extent; the same lines in
    numpy float32 are printed in that unit and do no better.  Measured worst: 1.12 units at B = 257 (a up to 12.2, raw error 4.1e-7;
    float32 numpy 1.12 units); bound 3 units, inside the 8 of the count."""
    lib, ptr, stream = _abi()
    rs = np.random.RandomState(300 + B + P)
    n_obj = min(B, 5)
    table = rand_mesh(rs, n_obj, P)
    obj = rs.randint(0, n_obj, B).astype(np.int32)
    boxes = rand_boxes(rs, B, 480, 640)
    K = rand_K(rs, 3 if with_im else B, 480, 640)
    im = rs.randint(0, 3, B).astype(np.int32) if with_im else None
    out = torch.full((B, 4, 4), 7.0, device='cuda')
    b_, t_, o_, K_, im_ = dev(boxes), dev(table), ints(obj), dev(K), ints(im)
    assert lib.cosy_tco_init_zup_autodepth(ptr(b_), ptr(t_), ptr(o_), ptr(K_), ptr(im_), B, P, ptr(out), stream()) == COSY_OK
    Kb = K if im is None else K[im]
    want, C = ref_tco_init_zup(boxes, table[obj], Kb)
    got = host(out)
    rot, tr = pose_err(got, want)
    assert rot.max() == 0.0
    if P == 1:
        assert np.array_equal(got.astype(np.float64), want)
        print('  P=1: exact (depth 0)')
        return
    ext = np.stack([C[:, :, 0].max(1) - C[:, :, 0].min(1), C[:, :, 1].max(1) - C[:, :, 1].min(1)], 1)
    a = (np.abs(C[:, :, :2]).max(1) / ext).max(1)
    _, tr32 = pose_err(ref_tco_init_zup(boxes, table[obj], Kb, np.float32)[0], want)
    print(f'  B={B} P={P}: a = {a.min():.3g} .. {a.max():.3g}; raw error {tr.max():.3g}; float32 numpy in the unit {float((tr32 / (U32 * (1 + a))).max()):.3g}')
    report(f'B={B} P={P} im_id={int(with_im)} translation / (u32 (1 + a))', float((tr / (U32 * (1 + a))).max()), ZUP_C)


# ---------------------------------------------------------------------------------------------------------------------------
# segmented argmin, id expansion
# ---------------------------------------------------------------------------------------------------------------------------
def run_scatter_argmin(d, ids, n_seg):
    lib, ptr, stream = _abi()
    out = torch.full((n_seg + 1,), 7, dtype=torch.int32, device='cuda')
    d_, i_ = dev(d), ints(ids)
    assert lib.cosy_scatter_argmin(ptr(d_), ptr(i_), len(d), n_seg, ptr(out), stream()) == COSY_OK
    assert int(out[n_seg]) == 7
    return host(out[:n_seg])


@gpu
@pytest.mark.parametrize('M', [1, 37, 63, 64, 65, 130, 1000, 5000])
def test_scatter_argmin_exact(M):
    """cosy_scatter_argmin against the C++ loop's restatement, exactly (the values compared are the same float32 numbers on both
    sides, so no separation is needed): M < 64 and M % 64 != 0; unsorted ids; segments without a member (-1; the reference's
    C++ yields 0 there, see ref_scatter_argmin); continuous values; heavy exact ties (values 0 .. 2), where the first index must win
    within a lane (m and m + 64 share one) and across lanes; all values equal."""
    rs = np.random.RandomState(400 + M)
    n_seg = max(3, M // 7)
    ids = rs.randint(0, n_seg, M).astype(np.int32)
    ids[ids == 1] = 0                                                          # segment 1 has no member ...
    n_seg += 2                                                                 # ... nor have the last two
    for tag, d in (('continuous', rs.randn(M)), ('ties', rs.randint(0, 3, M)), ('equal', np.ones(M))):
        d = d.astype(np.float32)
        want = ref_scatter_argmin(d, ids, n_seg)
        assert want[1] == -1 and want[-1] == -1
        got = run_scatter_argmin(d, ids, n_seg)
        print(f'  M={M} {tag}: {int((got != want).sum())} of {n_seg} segments differ')
        assert np.array_equal(got, want)
    one = np.zeros(M, np.int32)                                                # one segment of M members, ties 64 apart
    d = (np.arange(M) % 64 // 32).astype(np.float32)[::-1].copy()
    assert np.array_equal(run_scatter_argmin(d, one, 1), ref_scatter_argmin(d, one, 1))


@gpu
def test_scatter_argmin_nan_follows_the_reference_scan():
    """The reference's loop seeds a segment's minimum with its first member and replaces it on `value < lowest`: a NaN first member
    is never replaced, a later NaN never chosen.  Segments of 200 members with the NaN first, in the middle (another lane), last,
    everywhere, and everywhere but one."""
    n = 200
    d = np.tile(np.linspace(1.0, 2.0, n, dtype=np.float32)[::-1], (5, 1))
    d[0, 0] = np.nan; d[1, 77] = np.nan; d[2, n - 1] = np.nan; d[3, :] = np.nan; d[4, :] = np.nan; d[4, 150] = 3.0
    ids = np.repeat(np.arange(5, dtype=np.int32), n)
    perm = np.random.RandomState(5).permutation(5 * n)                          # unsorted ids
    dd, ii = d.reshape(-1)[perm], ids[perm]
    want = ref_scatter_argmin(dd, ii, 5)
    got = run_scatter_argmin(dd, ii, 5)
    print(f'  NaN segments: kernel {got.tolist()} reference {want.tolist()}')
    assert np.array_equal(got, want)
    want = ref_scatter_argmin(d.reshape(-1), ids, 5)
    assert want.tolist() == [0, 2 * n - 1, 3 * n - 2, 3 * n, 4 * n]             # first-is-NaN stays; otherwise the smallest number
    assert np.array_equal(run_scatter_argmin(d.reshape(-1), ids, 5), want)


@gpu
@pytest.mark.parametrize('B', [1, 255, 256, 257, 1000])
def test_expand_ids_exact(B):
    """cosy_expand_ids_for_symmetry around the 256-item scan block: counts 0 .. 6 with zeros, all zeros, all ones; the total."""
    lib, ptr, stream = _abi()
    rs = np.random.RandomState(500 + B)
    for tag, n in (('mixed', rs.randint(0, 7, B)), ('zeros', np.zeros(B)), ('ones', np.ones(B)), ('sparse', (rs.rand(B) < 0.05) * 6)):
        n = n.astype(np.int32)
        wa, wb = ref_expand_ids(n.tolist())
        M = int(n.sum())
        a, b = (torch.full((M + 1,), -7, dtype=torch.int32, device='cuda') for _ in range(2))
        total = torch.full((1,), -7, dtype=torch.int32, device='cuda')
        n_ = ints(n)
        assert lib.cosy_expand_ids_for_symmetry(ptr(n_), B, ptr(a), ptr(b), ptr(total), stream()) == COSY_OK
        print(f'  B={B} {tag}: M = {M}')
        assert int(total) == M and int(a[M]) == -7 and int(b[M]) == -7
        assert np.array_equal(host(a[:M]), wa) and np.array_equal(host(b[:M]), wb)


# ---------------------------------------------------------------------------------------------------------------------------
# symmetric distance
# ---------------------------------------------------------------------------------------------------------------------------
# Real-valued distance results: two figures per case, both per item.
#   relative: |got - want| / want over the items whose distance is at least 1 % of Z, the largest translation entry of the two poses
#             (nothing cancels there: what is seen is the order of the P-term sum);
#   absolute: |got - want| / Z over all items.  A distance of a millimetre between two point sets a metre away is the difference of
#             coordinates rounded at u32 x 1 m, so its error relative to ITSELF is ~1e-4 whatever the kernel does; relative to the
#             coordinates it is a few u32.  (The reference's float32 has the same floor.)
# Measured worst on an MI355X: relative 1.96e-6 (symmetric distance, B = 257, mode 1), 1.64e-6 (loss_co_symmetric, P = 1), 1.78e-6
# (disentangled loss, B = 257); absolute 3.6e-8 (symmetric distance, P = 1), 1.9e-8 (loss), 3.7e-8 (disentangled loss).
DIST_REL_TOL = 5e-6       # half of test_gpu_parity.py's DIST_TOL
DIST_ABS_TOL = 1e-7       # < 2 u32; a count of roundings allows 16 u32 (two transforms, 6 roundings of magnitude Z per coordinate)


def dist_figures(got, want, Z):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want)
    big = want >= 0.01 * Z
    return (float((err[big] / want[big]).max()) if big.any() else 0.0), float((err / Z).max())


def report_dist(tag, got, want, Z):
    rel, ab = dist_figures(got, want, Z)
    report(f'{tag} relative', rel, DIST_REL_TOL)
    report(f'{tag} absolute / Z', ab, DIST_ABS_TOL)


def pose_scale(*Ts):
    return np.max([np.abs(np.asarray(T, np.float64)[:, :3, 3]).max(1) for T in Ts], axis=0)


def run_symmetric_distance(c, mode, use_nsym=True, sel=None):
    lib, ptr, stream = _abi()
    sel = np.arange(len(c['T1'])) if sel is None else np.asarray(sel)
    B, P, S = len(sel), c['table'].shape[1], c['sym'].shape[1]
    if c['rows']:                                                # obj_id null: the tables are per item
        t, s, n, o = dev(c['table'][sel]), dev(c['sym'][sel]), ints(c['n_sym'][sel]), None
    else:
        t, s, n, o = dev(c['table']), dev(c['sym']), ints(c['n_sym']), ints(c['obj'][sel])
    T1, T2 = dev(c['T1'][sel]), dev(c['T2'][sel])
    d = torch.full((B,), 7.0, device='cuda'); best = torch.full((B,), 7, dtype=torch.int32, device='cuda'); S12 = torch.full((B, 4, 4), 7.0, device='cuda')
    rc = lib.cosy_symmetric_distance(ptr(T1), ptr(T2), ptr(o), ptr(t), ptr(s), ptr(n) if use_nsym else None, B, P, S, mode, ptr(d), ptr(best),
                                     ptr(S12), stream())
    assert rc == COSY_OK, lib.cosy_last_error()
    return d, best, S12


@gpu
@pytest.mark.parametrize('name', list(SD_CASES))
@pytest.mark.parametrize('mode', [0, 1])
def test_symmetric_distance_vs_fp64(name, mode):
    """cosy_symmetric_distance, both modes: P = 1 .. 2000 around the 256-thread tails, S = 1 .. 64, B = 1 .. 257, obj_id given and
    null (item b = table row b), mode 0 over the n_sym real rows, mode 1 over the identity-padded table (when row 0 is the best,
    the padding ties with it exactly and row 0 must win), mode 0 with n_sym null (all S rows), and a table whose rows past n_sym hold
    other rotations that fit better than any real row (mode 0 must not scan them, mode 1 must).  best_sym and S12 exact for every
    item; the cases are separated (sd_expect).  Run twice: bit-identical; items 0, B/2 and B-1 alone (B = 1): bit-identical to
    their values in the batch."""
    c = sd_case(name)
    want_d, want_best, want_S12 = sd_expect(c, mode)
    d, best, S12 = run_symmetric_distance(c, mode)
    Z = pose_scale(c['T1'], c['T2'])
    print(f'  {name} mode {mode}: best_sym differs in {int((host(best) != want_best).sum())} of {len(want_best)} items; distances {want_d.min():.3g} .. {want_d.max():.3g} m')
    assert np.array_equal(host(best), want_best)
    assert np.array_equal(host(S12), want_S12)
    report_dist(f'{name} mode {mode}', host(d), want_d, Z)
    d2, best2, S122 = run_symmetric_distance(c, mode)
    assert torch.equal(d, d2) and torch.equal(best, best2) and torch.equal(S12, S122)
    for b in sorted({0, len(want_d) // 2, len(want_d) - 1}):
        d1, b1, s1 = run_symmetric_distance(c, mode, sel=[b])
        assert torch.equal(d1[0], d[b]) and torch.equal(b1[0], best[b]) and torch.equal(s1[0], S12[b])
    if mode == 0 and name in ('padded', 'P2000'):                              # n_sym null: mode 0 falls back to all S rows
        wd, wb, ws = sd_expect(c, 0, use_nsym=False)
        d, best, S12 = run_symmetric_distance(c, 0, use_nsym=False)
        assert np.array_equal(host(best), wb) and np.array_equal(host(S12), ws)
        report_dist(f'{name} mode 0, n_sym null', host(d), wd, Z)


@gpu
def test_symmetric_distance_nan_pose():
    """A NaN in one item's T1: every cost of that item is NaN.  The reference's argmin (mode 1) and its C++ scan (mode 0) both end on
    index 0 then, with a NaN distance; the other items are bit-identical to the clean run."""
    c = sd_case('P257')
    for mode in (0, 1):
        clean = run_symmetric_distance(c, mode)
        bad = dict(c, T1=c['T1'].copy()); bad['T1'][2, 1, 3] = np.nan
        d, best, S12 = run_symmetric_distance(bad, mode)
        keep = torch.tensor([0, 1, 3, 4], device='cuda')
        assert all(torch.equal(a[keep], b[keep]) for a, b in zip((d, best, S12), clean))
        assert bool(torch.isnan(d[2])) and int(best[2]) == 0
        assert np.array_equal(host(S12[2]), c['sym'][c['obj'][2], 0])


# ---------------------------------------------------------------------------------------------------------------------------
# losses
# ---------------------------------------------------------------------------------------------------------------------------
def run_loss_co(c, gathered, want_ids=True, sel=None):
    """gathered: points (B,P,3) with obj_id null (what lib3d passes); else the table with obj_id"""
    lib, ptr, stream = _abi()
    sel = np.arange(len(c['pred'])) if sel is None else np.asarray(sel)
    B, S, P = len(sel), c['gt'].shape[1], c['table'].shape[1]
    t, o = (dev(c['table'][c['obj'][sel]]), None) if gathered else (dev(c['table']), ints(c['obj'][sel]))
    gt, pred = dev(c['gt'][sel]), dev(c['pred'][sel])
    loss = torch.full((B,), 7.0, device='cuda'); mid = torch.full((B,), 7, dtype=torch.int32, device='cuda'); assign = torch.full((B, 4, 4), 7.0, device='cuda')
    rc = lib.cosy_loss_co_symmetric(ptr(gt), ptr(pred), ptr(t), ptr(o), B, S, P, ptr(loss), ptr(mid) if want_ids else None,
                                    ptr(assign) if want_ids else None, stream())
    assert rc == COSY_OK, lib.cosy_last_error()
    return loss, mid, assign


@gpu
@pytest.mark.parametrize('name', list(LOSS_CASES))
def test_loss_co_symmetric_vs_fp64(name):
    """cosy_loss_co_symmetric: P = 1 .. 2000 around the 256-thread tails, S = 1 / 4 / 8, B = 1 .. 257; points gathered per item
    (obj_id null) and through the object table (obj_id given): bit-identical; min_id and TCO_assign null: the loss is bit-identical
    and nothing is written.  min_id / TCO_assign exact for every item: separated cases, with ground truth 2 a bitwise copy of 0 (and
    the identity-padded symmetries) as exact ties that the first must win.  Twice and item-alone: bit-identical."""
    c = loss_case(name)
    want_l, want_id = loss_expect(c)
    loss, mid, assign = run_loss_co(c, gathered=False)
    print(f'  {name}: min_id differs in {int((host(mid) != want_id).sum())} of {len(want_id)} items; ties in {int((first_identical(c["gt"]).max(1) < c["gt"].shape[1] - 1).sum())}')
    assert np.array_equal(host(mid), want_id)
    assert np.array_equal(host(assign), c['gt'][np.arange(len(want_id)), want_id])
    report_dist(f'{name} loss', host(loss), want_l, pose_scale(c['pred'], c['gt'][:, 0]))
    l2, m2, a2 = run_loss_co(c, gathered=True)
    assert torch.equal(loss, l2) and torch.equal(mid, m2) and torch.equal(assign, a2)
    l3, m3, a3 = run_loss_co(c, gathered=False, want_ids=False)
    assert torch.equal(loss, l3) and bool((m3 == 7).all()) and bool((a3 == 7.0).all())
    for b in sorted({0, len(want_l) // 2, len(want_l) - 1}):
        l1, m1, a1 = run_loss_co(c, gathered=False, sel=[b])
        assert torch.equal(l1[0], loss[b]) and torch.equal(m1[0], mid[b]) and torch.equal(a1[0], assign[b])


def run_disentangled(c, gathered=False, sel=None):
    lib, ptr, stream = _abi()
    sel = np.arange(len(c['Tin'])) if sel is None else np.asarray(sel)
    B, S, P = len(sel), c['gt'].shape[1], c['table'].shape[1]
    t, o = (dev(c['table'][c['obj'][sel]]), None) if gathered else (dev(c['table']), ints(c['obj'][sel]))
    gt, Tin, o9, K = dev(c['gt'][sel]), dev(c['Tin'][sel]), dev(c['out9'][sel]), dev(c['K'][sel])
    loss = torch.full((B,), 7.0, device='cuda')
    rc = lib.cosy_loss_refiner_disentangled(ptr(gt), ptr(Tin), ptr(o9), ptr(K), ptr(t), ptr(o), B, S, P, ptr(loss), stream())
    assert rc == COSY_OK, lib.cosy_last_error()
    return loss


@gpu
@pytest.mark.parametrize('name', list(LOSS_CASES))
def test_loss_refiner_disentangled_vs_fp64(name):
    """cosy_loss_refiner_disentangled on the loss cases (K_crop with fy = 0.7 .. 1.3 fx), table and gathered form bit-identical,
    twice and item-alone bit-identical."""
    c = loss_case(name)
    want, _ = ref_disentangled(c['gt'], c['Tin'], c['out9'], c['K'], c['table'][c['obj']])
    loss = run_disentangled(c)
    report_dist(f'{name} disentangled', host(loss), want, pose_scale(c['Tin'], c['gt'][:, 0]))
    assert torch.equal(loss, run_disentangled(c)) and torch.equal(loss, run_disentangled(c, gathered=True))
    for b in sorted({0, len(want) // 2, len(want) - 1}):
        assert torch.equal(run_disentangled(c, sel=[b])[0], loss[b])


@gpu
@pytest.mark.parametrize('term', ['orientation', 'xy', 'z'])
def test_loss_refiner_disentangled_one_term_alone(term):
    """Each term on its own: inputs for which the two other predictions equal ground truth 0 bit for bit, so their minima are exactly
    0 and the loss IS the remaining term.  (Identity update (1,0,0,0,1,0) -> dR = I exactly; an input pose on the optical axis with
    v = 0 -> xy = (0 / f + 0 / z) z = 0 exactly; vz = 1 -> z kept exactly.)  S = 3 with two far ground truths behind the first."""
    rs = np.random.RandomState(600)
    B, P = 9, 300
    table = rand_mesh(rs, B, P)
    g0 = rand_poses(rs, B); g0[:, :2, 3] = 0
    far = lambda: np.stack([(g0[b].astype(np.float64) @ small_motion(rs, rot=0.3, trans=0.1)) for b in range(B)]).astype(np.float32)
    gt = np.stack([g0, far(), far()], 1)
    Tin = g0.copy()
    out9 = np.tile(np.float32([1, 0, 0, 0, 1, 0, 0, 0, 1]), (B, 1))
    K = rand_K(rs, B, 240, 320); K[:, 1, 1] = K[:, 0, 0] * np.float32(1.25)
    if term == 'orientation':
        out9[:, :6] += (rs.randn(B, 6) * 0.2).astype(np.float32)
    elif term == 'xy':
        out9[:, 6:8] = (rs.randn(B, 2) * 20).astype(np.float32)
    else:
        out9[:, 8] = rs.uniform(0.7, 1.4, B)
    c = dict(table=table, obj=np.arange(B, dtype=np.int32), gt=gt, Tin=Tin, out9=out9, K=K)
    want, tabs = ref_disentangled(gt, Tin, out9, K, table)
    others = [t for t, n in zip(tabs, ('orientation', 'xy', 'z')) if n != term]
    assert all((t.min(1) == 0).all() for t in others) and (want > 1e-4).all()
    report_dist(f'{term} alone', host(run_disentangled(c)), want, pose_scale(Tin))


@gpu
def test_loss_refiner_disentangled_terms_choose_different_ground_truths():
    """S = 3 where the orientation term is assigned ground truth 1, the xy term 0 and the depth term 2 (asserted in float64 by
    test_index_case_preconditions): a kernel that reuses one term's assignment for another, or the first ground truth for all, is
    off by centimetres."""
    c = disentangled_per_term_case()
    want, tabs = ref_disentangled(c['gt'], c['Tin'], c['out9'], c['K'], c['table'][c['obj']])
    shared = sum(tabs).min(1)                                                   # one assignment for the sum of the terms
    assert ((shared - want) / want > 1e-2).all()
    report_dist('per-term ground truths', host(run_disentangled(c)), want, pose_scale(c['Tin']))


@gpu
def test_losses_nan_follow_torch_min():
    """torch.min / argmin take a NaN as the minimum (the first one).  A NaN prediction: every cost is NaN -> loss NaN, min_id 0.  A NaN
    in ground truth 2 only: torch.min returns that NaN and index 2 although finite costs exist.  Other items: bit-identical."""
    c = loss_case('P257')
    clean = run_loss_co(c, gathered=False)
    bad = dict(c, pred=c['pred'].copy(), gt=c['gt'].copy())
    bad['pred'][1, 0, 0] = np.nan
    bad['gt'][3, 1, 2, 3] = np.nan
    loss, mid, assign = run_loss_co(bad, gathered=False)
    t = torch.from_numpy(ref_loss_co_costs(bad['gt'], bad['pred'], bad['table'][bad['obj']]))
    tl, ti = t.min(dim=1)
    print(f'  torch.min on the float64 costs: min_id {ti.tolist()}; kernel {host(mid).tolist()}')
    assert ti.tolist()[1] == 0 and ti.tolist()[3] == 1 and bool(torch.isnan(tl[1])) and bool(torch.isnan(tl[3]))
    assert np.array_equal(host(mid), ti.numpy().astype(np.int32))
    assert bool(torch.isnan(loss[1])) and bool(torch.isnan(loss[3]))
    keep = torch.tensor([0, 2, 4], device='cuda')
    assert all(torch.equal(a[keep], b[keep]) for a, b in zip((loss, mid, assign), clean))
    dl = run_disentangled(dict(bad, Tin=bad['pred'], gt=c['gt']))
    dc = run_disentangled(dict(c, Tin=c['pred']))
    assert bool(torch.isnan(dl[1])) and torch.equal(dl[keep], dc[keep]) and torch.equal(dl[3], dc[3])


# ---------------------------------------------------------------------------------------------------------------------------
# ADD / ADD-S
# ---------------------------------------------------------------------------------------------------------------------------
ADD_TOL = 4e-7            # residual vectors and norms, absolute / Z per item (measured worst 1.42e-7 ADD, 1.32e-7 ADD-S; a count allows 13 u32 = 7.7e-7)


def run_dists_add(pts, Tp, Tg, symmetric, obj=None):
    lib, ptr, stream = _abi()
    B, P = len(Tp), pts.shape[1]
    out = torch.full((B + 1, P, 3), 7.0, device='cuda')
    p_, a_, g_, o_ = dev(pts), dev(Tp), dev(Tg), ints(obj)
    assert lib.cosy_dists_add(ptr(a_), ptr(g_), ptr(p_), ptr(o_), B, P, symmetric, ptr(out), stream()) == COSY_OK
    assert bool((out[B] == 7.0).all())
    return out[:B]


@gpu
@pytest.mark.parametrize('B,P', [(1, 1), (3, 255), (3, 256), (3, 257), (2, 2049), (257, 70)])
def test_dists_add_vs_fp64(B, P):
    """cosy_dists_add, ADD form: residual vectors per item against |t|; points per item and through a shuffled object table
    bit-identical; twice bit-identical; item alone bit-identical."""
    rs = np.random.RandomState(700 + B + P)
    n_obj = min(B, 4)
    table = rand_mesh(rs, n_obj, P)
    obj = rs.randint(0, n_obj, B).astype(np.int32)
    Tg = rand_poses(rs, B)
    Tp = np.stack([Tg[b].astype(np.float64) @ small_motion(rs, rot=0.1, trans=0.01) for b in range(B)]).astype(np.float32)
    want = ref_dists_add(Tp, Tg, table[obj])
    got = run_dists_add(table, Tp, Tg, 0, obj)
    Z = pose_scale(Tp, Tg)
    report(f'B={B} P={P} ADD vectors / Z', float((np.abs(host(got) - want).reshape(B, -1).max(1) / Z).max()), ADD_TOL)
    assert torch.equal(got, run_dists_add(table[obj], Tp, Tg, 0)) and torch.equal(got, run_dists_add(table, Tp, Tg, 0, obj))
    assert torch.equal(run_dists_add(table, Tp[-1:], Tg[-1:], 0, obj[-1:])[0], got[-1])


@gpu
@pytest.mark.parametrize('name', list(ADDS_CASES))
def test_dists_add_symmetric_vs_fp64(name):
    """cosy_dists_add, ADD-S form, at P < 256 and the 2048-point chunk boundaries, with duplicated mesh points.
    Residual NORMS at every point (the nearest distance is continuous in the inputs, whichever neighbour a float32 kernel picks);
    residual VECTORS at the points whose float64 nearest and second-nearest predicted points (duplicates counted once) differ in
    distance by more than ADDS_SEP_MULT x the float32 bound of one distance; the excluded share is asserted <= 1 %.
    Twice: bit-identical; the last item alone: bit-identical."""
    c = adds_case(name)
    want, sep, _ = adds_expect(c)
    excluded = int((~sep).sum(axis=1).max())
    assert excluded <= ADDS_MAX_EXCLUDED * sep.shape[1]
    got = run_dists_add(c['pts'], c['Tp'], c['Tg'], 1)
    g = host(got).astype(np.float64)
    Z = pose_scale(c['Tp'], c['Tg'])
    print(f'  {name}: {excluded} of {sep.shape[1]} points excluded from the vector comparison')
    report(f'{name} ADD-S norms / Z', float((np.abs(np.linalg.norm(g, axis=-1) - np.linalg.norm(want, axis=-1)).max(1) / Z).max()), ADD_TOL)
    report(f'{name} ADD-S vectors (separated points) / Z', float(((np.abs(g - want).max(-1) * sep).max(1) / Z).max()), ADD_TOL)
    assert torch.equal(got, run_dists_add(c['pts'], c['Tp'], c['Tg'], 1))
    assert torch.equal(run_dists_add(c['pts'][-1:], c['Tp'][-1:], c['Tg'][-1:], 1)[0], got[-1])


# ---------------------------------------------------------------------------------------------------------------------------
# frame repacking (exact)
# ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('N,h,w', [(1, 13, 17), (3, 13, 17), (1, 16, 16), (3, 30, 41), (1, 1, 1)])
def test_frames_to_nhwc4_exact(N, h, w):
    """cosy_frames_to_nhwc4 / cosy_frames_u8_to_nhwc4 at h * w % 256 != 0 (and == 0), N = 1 / 3: channel 3 is 0, the rest the
    frame's values (uint8: value / 255 in float32, the reference's images.float() / 255., evaluated on the CPU: a true division)."""
    lib, ptr, stream = _abi()
    g = torch.Generator().manual_seed(N * 1000 + h * w)
    x = torch.randn(N, 3, h, w, generator=g).cuda()
    u = torch.randint(0, 256, (N, 3, h, w), generator=g, dtype=torch.uint8).cuda()
    for tag, fn, src, ref in (('fp32', lib.cosy_frames_to_nhwc4, x, x), ('uint8', lib.cosy_frames_u8_to_nhwc4, u, (u.cpu().float() / 255.).cuda())):
        out = torch.full((N * h * w + 1, 4), 7.0, device='cuda')
        assert fn(ptr(src), ptr(out), N, h, w, stream()) == COSY_OK
        want = torch.cat([ref.permute(0, 2, 3, 1), torch.zeros(N, h, w, 1, device='cuda')], -1).reshape(-1, 4)
        print(f'  N={N} {h}x{w} {tag}: {int((out[:-1] != want).sum())} elements differ')
        assert torch.equal(out[:-1], want) and bool((out[-1] == 7.0).all())


# ---------------------------------------------------------------------------------------------------------------------------
# wrapper contracts: refused on the host, nothing launched
# ---------------------------------------------------------------------------------------------------------------------------
def _contract_calls(pin, pout):
    """entry -> (function name, good arguments in ABI order, names of the optional pointers).  pin: a zeroed device buffer that is only
    read (every id in it is 0); pout: another one that every output goes to.  Both are far larger than any good call at these sizes."""
    return {
        'crop_geometry': ('cosy_crop_geometry', dict(pts_table=pin, obj_id=pin, K=pin, im_id=None, TCO=pin, B=2, P=3, z_min=Z_MIN, im_h=48, im_w=64,
                                                     out_h=24, out_w=32, lamb=LAMB, boxes_rend=pout, boxes_crop=pout, K_crop=pout), ('im_id',)),
        'roi_align': ('cosy_roi_align', dict(images=pin, im_id=None, boxes=pin, B=2, N=2, C=3, h=8, w=8, out_h=1, out_w=1, sampling_ratio=4, out=pout),
                      ('im_id',)),
        'pose_update': ('cosy_pose_update', dict(TCO_in=pin, K_crop=pin, pose9=pin, B=2, TCO_out=pout), ()),
        'tco_init_from_boxes': ('cosy_tco_init_from_boxes', dict(boxes=pin, K=pin, im_id=None, B=2, z=1.0, TCO=pout), ('im_id',)),
        'tco_init_zup_autodepth': ('cosy_tco_init_zup_autodepth', dict(boxes=pin, pts_table=pin, obj_id=pin, K=pin, im_id=None, B=2, P=3, TCO=pout),
                                   ('im_id',)),
        'scatter_argmin': ('cosy_scatter_argmin', dict(dists=pin, ids=pin, M=4, n_seg=2, out=pout), ()),
        'expand_ids_for_symmetry': ('cosy_expand_ids_for_symmetry', dict(n_sym_item=pin, B=2, ids_expand=pout, sym_ids=pout, total=None), ('total',)),
        'symmetric_distance': ('cosy_symmetric_distance', dict(T1=pin, T2=pin, obj_id=None, pts_table=pin, sym_table=pin, n_sym=None, B=2, P=3, S=1,
                                                               mode=0, min_dists=pout, best_sym=pout, S12=pout), ('obj_id', 'n_sym')),
        'loss_co_symmetric': ('cosy_loss_co_symmetric', dict(TCO_possible_gt=pin, TCO_pred=pin, pts_table=pin, obj_id=None, B=2, S=1, P=3, loss=pout,
                                                             min_id=None, TCO_assign=None), ('obj_id', 'min_id', 'TCO_assign')),
        'loss_refiner_disentangled': ('cosy_loss_refiner_disentangled', dict(TCO_possible_gt=pin, TCO_input=pin, refiner_outputs=pin, K_crop=pin,
                                                                             pts_table=pin, obj_id=None, B=2, S=1, P=3, loss=pout), ('obj_id',)),
        'dists_add': ('cosy_dists_add', dict(TXO_pred=pin, TXO_gt=pin, pts_table=pin, obj_id=None, B=2, P=1, symmetric=1, dists=pout), ('obj_id',)),
        'frames_to_nhwc4': ('cosy_frames_to_nhwc4', dict(images=pin, out=pout, N=2, h=1, w=1), ()),
        'frames_u8_to_nhwc4': ('cosy_frames_u8_to_nhwc4', dict(images=pin, out=pout, N=2, h=1, w=1), ()),
    }


_SIZE_ARGS = ('B', 'N', 'M', 'n_seg', 'P', 'S', 'C', 'h', 'w', 'im_h', 'im_w', 'out_h', 'out_w', 'sampling_ratio')
_ZERO_REFUSED = ('P', 'S', 'C', 'h', 'w', 'im_h', 'im_w', 'out_h', 'out_w', 'sampling_ratio')       # (an empty batch and M = 0 are valid)
_BATCH_ARG = {'scatter_argmin': 'n_seg', 'frames_to_nhwc4': 'N', 'frames_u8_to_nhwc4': 'N'}
_GRID_Y = {'roi_align': 'B', 'dists_add': 'B', 'frames_to_nhwc4': 'N', 'frames_u8_to_nhwc4': 'N'}       # the batch rides in gridDim.y
CONTRACT_ENTRIES = ['crop_geometry', 'roi_align', 'pose_update', 'tco_init_from_boxes', 'tco_init_zup_autodepth', 'scatter_argmin',
                    'expand_ids_for_symmetry', 'symmetric_distance', 'loss_co_symmetric', 'loss_refiner_disentangled', 'dists_add',
                    'frames_to_nhwc4', 'frames_u8_to_nhwc4']


@gpu
@pytest.mark.parametrize('entry', CONTRACT_ENTRIES)
def test_wrapper_contract(entry):
    """Every entry refuses, with COSY_EINVAL and a cosy_last_error() that names the argument ("P=0", "null TCO"), before anything is
    launched: each required pointer null; each size negative; P, S, C, h, w, the frame and crop sizes and sampling_ratio 0; a batch
    of 65536 where the batch is the grid's y dimension (65535 is the hardware's limit; the launch would otherwise fail inside the
    runtime).  An empty batch returns COSY_OK with every data pointer null.  The good call itself returns COSY_OK.  The output
    buffer is untouched by every refused call."""
    lib, ptr, stream = _abi()
    inb, outb = torch.zeros(1 << 15, device='cuda'), torch.zeros(1 << 15, device='cuda')
    fname, good, optional = _contract_calls(inb.data_ptr(), outb.data_ptr())[entry]
    fn = getattr(lib, fname)
    batch = _BATCH_ARG.get(entry, 'B')
    pointers = [k for k, v in good.items() if k not in _SIZE_ARGS and (v is None or v in (inb.data_ptr(), outb.data_ptr()))]

    def call(**over):
        return fn(*dict(good, **over).values(), stream())

    def refused(what, needle, **over):
        rc = call(**over)
        msg = lib.cosy_last_error().decode()
        print(f'  {entry} {what}: rc {rc}, "{msg}"')
        assert rc == COSY_EINVAL, (entry, what, rc)
        assert needle in msg, (entry, what, msg)

    assert call() == COSY_OK, lib.cosy_last_error()
    torch.cuda.synchronize()
    outb.zero_()
    torch.cuda.synchronize()
    for name in good:
        if name in _SIZE_ARGS:
            refused(f'{name} = -1', f'{name}=-1', **{name: -1})
            if name in _ZERO_REFUSED:
                refused(f'{name} = 0', f'{name}=0', **{name: 0})
        elif name in pointers and name not in optional:
            refused(f'{name} = null', f'null {name}', **{name: None})
    if entry in _GRID_Y:
        refused(f'{_GRID_Y[entry]} = 65536', f'{_GRID_Y[entry]}=65536', **{_GRID_Y[entry]: 65536})
    assert call(**dict({k: None for k in pointers}, **{batch: 0})) == COSY_OK, lib.cosy_last_error()
    torch.cuda.synchronize()
    assert bool((outb == 0).all()) and bool((inb == 0).all())                   # no refused call wrote anything
