"""Pose evaluation on the GPU: distances.pose_errors (csrc/kernels_eval.hip) and PoseErrorMeter end to end.

Yardsticks and bounds (u = 2^-24, the unit roundoff of float32; every test prints its figures before it asserts):

1. A float64 numpy evaluation of the reference formula (ref64 below).  The device works in float32, so the bound follows from the
   arithmetic.  A transformed coordinate ((a x + b y) + c z) + t carries three products and three sums: its error is at most
   E = 5 u S, S = max(|a x| + |b y| + |c z| + |t|) over the points and both poses (4 u S to first order; 5 covers the higher orders).
   A per-point vector g - q is off by at most 2 E + u |g - q| per component, i.e. its end points move by at most delta =
   2 sqrt(3) E; a nearest-point DISTANCE moves by no more than the points do.  Hence
       |norm_avg - ref| <= delta + 5 u ref                                    (5 u: bound 2 below),
   and, because xyz_avg of ADD-S is discontinuous where two predicted points are nearly equally near, xyz_avg is checked against
   an INTERVAL: ref64 takes, per ground-truth point, the smallest and largest |component| over every predicted point whose
   distance is within 2 delta of the minimum (for ADD: the one pair), and mean(lo) - tol <= xyz_avg <= mean(hi) + tol with
   tol = 2 E + 5 u hi.
2. distances.dists_add / dists_add_symmetric on the same inputs, reduced in float64.  The per-point vectors are the same bits, so
   what differs is: the squared norm (dx dx + dy dy) + dz dz in float32 (three roundings on a sum of non-negative terms: 3 u on
   the square, 1.5 u on the root), one float32 sqrt (at most 1 ulp = 2 u; 1 u where it is correctly rounded), float64 sums
   (negligible) and the final rounding to float32 (u): 4.5 u.  DERIVED_ULPS = 5, on norm_avg and xyz_avg alike.
3. The reference's own float32 errors in the fixture: the larger of bound 2 and twice the reference's recorded
   float32-vs-float64 deviation of that field (tests/golden/generate_golden_eval.py records it).
The meter's tables must equal the recorded ones exactly (the generator asserts that no decision is within 1e-3 of flipping);
the summary's counts, ratios, AP and mAP to 1e-12; its error means within bound 3; the AUCs within bound 3 taken absolutely
(AUC = 10 (0.1 a_n - mean of the errors below 0.1), so it moves by at most 10 x 0.1 x the relative bound).
"""
import numpy as np
import pandas as pd
import pytest
import torch

import pose_meter_case as pc

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
DERIVED_ULPS = 5
CHUNK = 2048          # EVAL_CHUNK of kernels_eval.hip: predicted points per LDS pass
TILE = 1024           # EVAL_TILE: ground-truth points per work item


def rand_pose(rs, n, t_scale=0.5):
    q = rs.normal(size=(n, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    T = np.tile(np.eye(4), (n, 1, 1))
    T[:, :3, :3] = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                             2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1).reshape(n, 3, 3)
    T[:, :3, 3] = rs.uniform(-t_scale, t_scale, (n, 3)) + np.array([0, 0, 1.0])
    return T.astype(np.float32)


def near_pose(rs, T, angle=0.05, trans=0.01):
    """T . (small rotation, small translation): a prediction near the ground truth, so that nearest points are contested"""
    out = T.astype(np.float64).copy()
    for n in range(len(T)):
        axis = rs.normal(size=3); axis /= np.linalg.norm(axis)
        a = rs.normal() * angle
        K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        D = np.eye(4); D[:3, :3] = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K); D[:3, 3] = rs.normal(size=3) * trans
        out[n] = out[n] @ D
    return out.astype(np.float32)


def ref64(Tp, Tg, pts, symmetric, rows=256):
    """the reference formula (pose_meters.py:53-92, lib3d/distances.py) in float64 for ONE pair -> norm_avg, lo (3), hi (3), TCO_xyz,
    TCO_norm, E: see the module docstring (lo = hi = xyz_avg for ADD)"""
    Tp, Tg, p = Tp.astype(np.float64), Tg.astype(np.float64), pts.astype(np.float64)
    q, g = p @ Tp[:3, :3].T + Tp[:3, 3], p @ Tg[:3, :3].T + Tg[:3, 3]
    S = max((np.abs(p) @ np.abs(T[:3, :3]).T + np.abs(T[:3, 3])).max() for T in (Tp, Tg))
    E = 5 * U * S
    delta = 2 * np.sqrt(3) * E
    if not symmetric:
        d = g - q
        norm, lo, hi = np.linalg.norm(d, axis=1).mean(), np.abs(d).mean(0), np.abs(d).mean(0)
    else:
        norm, lo, hi = 0., np.zeros(3), np.zeros(3)
        for i0 in range(0, len(p), rows):
            d = g[i0:i0 + rows, None, :] - q[None, :, :]
            dist = np.sqrt(np.einsum('ijk,ijk->ij', d, d))
            dmin = dist.min(1)
            r, c = np.nonzero(dist <= dmin[:, None] + 2 * delta)          # the nearest point and whatever is nearly as near
            a = np.abs(d[r, c])
            lo_rows, hi_rows = np.full((len(dmin), 3), np.inf), np.zeros((len(dmin), 3))
            np.minimum.at(lo_rows, r, a)
            np.maximum.at(hi_rows, r, a)
            norm, lo, hi = norm + dmin.sum(), lo + lo_rows.sum(0), hi + hi_rows.sum(0)
        norm, lo, hi = norm / len(p), lo / len(p), hi / len(p)
    t = Tp[:3, 3] - Tg[:3, 3]
    return dict(norm_avg=norm, lo=lo, hi=hi, TCO_xyz=np.abs(t), TCO_norm=np.linalg.norm(t), E=E, delta=delta)


def ulps(got, want):
    """|got - want| in units of u |want| (0 where they are equal, zeros included)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.where(got == want, 0., np.abs(got - want) / np.maximum(U * np.abs(want), 1e-300))


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def run(Tp, Tg, obj, mode, table, n_points):
    from cosypose_amd.distances import pose_errors
    out = pose_errors(dev(Tp), dev(Tg), np.asarray(obj, np.int32), np.asarray(mode, np.int32), table if torch.is_tensor(table) else dev(table),
                      np.asarray(n_points, np.int32))
    torch.cuda.synchronize()
    return out


def via_dists(Tp, Tg, pts, symmetric):
    """the route the package offered before: the (1,P,3) vectors of dists_add / dists_add_symmetric, reduced in float64"""
    from cosypose_amd import distances
    fn = distances.dists_add_symmetric if symmetric else distances.dists_add
    d = fn(dev(Tp[None]), dev(Tg[None]), dev(pts[None])).double()
    return d.norm(dim=-1).mean(-1)[0].item(), d.abs().mean(-2)[0].cpu().numpy()


def check_pair(tag, got, b, Tp, Tg, pts, symmetric, worst):
    """one pair against yardsticks 1 and 2"""
    n, xyz = got['norm_avg'][b].item(), got['xyz_avg'][b].double().cpu().numpy()
    r = ref64(Tp, Tg, pts, symmetric)
    tol_n, tol_c = r['delta'] + DERIVED_ULPS * U * r['norm_avg'], 2 * r['E'] + DERIVED_ULPS * U * r['hi']
    dn, dxyz = via_dists(Tp, Tg, pts, symmetric)
    ulps_n, ulps_c = float(ulps(n, dn)), float(ulps(xyz, dxyz).max())
    worst['f64'] = max(worst.get('f64', 0.), abs(n - r['norm_avg']) / tol_n)
    worst['ulps'] = max(worst.get('ulps', 0.), ulps_n, ulps_c)
    print(f'{tag}: norm_avg {n:.9g} ref64 {r["norm_avg"]:.9g} (|diff| / bound {abs(n - r["norm_avg"]) / tol_n:.3f}); vs dists_add route '
          f'{ulps_n:.2f} u (norm) {ulps_c:.2f} u (xyz); xyz outside [lo, hi] by {np.max(np.maximum(np.maximum(r["lo"] - xyz, xyz - r["hi"]), 0) / tol_c):.3f} of its bound')
    assert abs(n - r['norm_avg']) <= tol_n
    assert np.all(xyz >= r['lo'] - tol_c) and np.all(xyz <= r['hi'] + tol_c)
    assert ulps_n <= DERIVED_ULPS and ulps_c <= DERIVED_ULPS
    assert np.allclose(got['TCO_xyz'][b].cpu().numpy(), r['TCO_xyz'], rtol=0, atol=2 * U * np.abs(np.stack([Tp, Tg])[:, :3, 3]).max())
    assert abs(got['TCO_norm'][b].item() - r['TCO_norm']) <= 4 * U * np.abs(np.stack([Tp, Tg])[:, :3, 3]).max() * np.sqrt(3)


SHAPES = [1, 255, 256, 257, TILE - 1, TILE, TILE + 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]


@pytest.mark.parametrize('P', SHAPES)
def test_pose_errors_shapes(P):
    """one object of P points, an ADD and an ADD-S pair with a prediction far from and one near the ground truth"""
    rs = np.random.RandomState(P)
    pts = (rs.uniform(-1, 1, (1, P, 3)) * rs.uniform(0.03, 0.12, 3)).astype(np.float32)
    Tg = rand_pose(rs, 4)
    Tp = np.concatenate([rand_pose(rs, 2), near_pose(rs, Tg[2:])])
    mode = [0, 1, 0, 1]
    got = run(Tp, Tg, [0] * 4, mode, pts, [P])
    worst = {}
    for b in range(4):
        check_pair(f'P={P} pair {b} mode {mode[b]}', got, b, Tp[b], Tg[b], pts[0], mode[b], worst)
    print('worst:', worst)


def test_pose_errors_large_mesh():
    """P >= 30 000 (15 LDS passes, 30 tiles): ADD-S with a prediction near the ground truth (contested nearest points), and ADD"""
    P = 30011
    rs = np.random.RandomState(7)
    pts = (rs.uniform(-1, 1, (1, P, 3)) * rs.uniform(0.03, 0.12, 3)).astype(np.float32)
    Tg = rand_pose(rs, 2)
    Tp = near_pose(rs, Tg)
    mode = [1, 0]
    got = run(Tp, Tg, [0] * 2, mode, pts, [P])
    worst = {}
    for b in range(2):
        check_pair(f'P={P} pair {b} mode {mode[b]}', got, b, Tp[b], Tg[b], pts[0], mode[b], worst)
    print('worst:', worst)


def mixed_batch(seed=11, B=40):
    rs = np.random.RandomState(seed)
    n_points = np.array([1, 37, 256, 700, 1025, 2049, 3000, 5000], dtype=np.int32)
    table = np.zeros((len(n_points), n_points.max(), 3), np.float32)
    for o, P in enumerate(n_points):
        table[o, :P] = rs.uniform(-1, 1, (P, 3)) * rs.uniform(0.03, 0.12, 3)
        table[o, P:] = 1e3                                  # padding far away: a read past n_points would show
    obj = rs.randint(0, len(n_points), B).astype(np.int32)
    mode = rs.randint(0, 2, B).astype(np.int32)
    Tg = rand_pose(rs, B)
    Tp = np.where((rs.uniform(size=B) < 0.5)[:, None, None], near_pose(rs, Tg), rand_pose(rs, B))
    return Tp, Tg, obj, mode, table, n_points


def test_mixed_sizes_and_modes_in_one_call():
    Tp, Tg, obj, mode, table, n_points = mixed_batch()
    got = run(Tp, Tg, obj, mode, table, n_points)
    worst = {}
    for b in range(len(obj)):
        check_pair(f'pair {b} P={n_points[obj[b]]} mode {mode[b]}', got, b, Tp[b], Tg[b], table[obj[b], :n_points[obj[b]]], mode[b], worst)
    print('worst:', worst)


def test_alone_equals_inside_a_batch_and_two_runs_are_equal():
    Tp, Tg, obj, mode, table, n_points = mixed_batch(seed=12)
    tab = dev(table)
    a, b = run(Tp, Tg, obj, mode, tab, n_points), run(Tp, Tg, obj, mode, tab, n_points)
    for k in pc.ERROR_FIELDS:
        assert torch.equal(a[k], b[k]), k
    for i in (0, 7, 19, len(obj) - 1):
        alone = run(Tp[i:i + 1], Tg[i:i + 1], obj[i:i + 1], mode[i:i + 1], tab, n_points)
        for k in pc.ERROR_FIELDS:
            assert torch.equal(alone[k][0], a[k][i]), (i, k)
    perm = np.random.RandomState(0).permutation(len(obj))
    c = run(Tp[perm], Tg[perm], obj[perm], mode[perm], tab, n_points)
    for k in pc.ERROR_FIELDS:
        assert torch.equal(c[k], a[k][torch.from_numpy(perm).cuda()]), k


def test_duplicated_points_first_minimum_wins():
    """every point three times: each nearest-point search has exact ties; the vectors must be those of dists_add_symmetric"""
    rs = np.random.RandomState(3)
    base = (rs.uniform(-1, 1, (300, 3)) * 0.1).astype(np.float32)
    pts = np.concatenate([base, base, base])[None]
    Tg = rand_pose(rs, 2)
    Tp = np.stack([Tg[0], near_pose(rs, Tg[1:])[0]])         # pair 0: identical poses, every distance 0 or tied
    got = run(Tp, Tg, [0, 0], [1, 1], pts, [900])
    worst = {}
    for b in range(2):
        check_pair(f'duplicates pair {b}', got, b, Tp[b], Tg[b], pts[0], 1, worst)
    assert got['norm_avg'][0].item() == 0.0 and not got['xyz_avg'][0].any()


def test_empty_batch():
    out = run(np.zeros((0, 4, 4), np.float32), np.zeros((0, 4, 4), np.float32), [], [], np.zeros((2, 5, 3), np.float32), [5, 5])
    assert out['norm_avg'].shape == (0,) and out['xyz_avg'].shape == (0, 3) and out['TCO_xyz'].shape == (0, 3) and out['TCO_norm'].shape == (0,)
    assert out['norm_avg'].is_cuda


def test_batch_beyond_a_grid_dimension():
    """B = 70 000 pairs of small meshes (the batch of cosy_dists_add rides gridDim.y and stops at 65 535)"""
    B, rs = 70000, np.random.RandomState(5)
    n_points = np.array([8, 5, 3], np.int32)
    table = (rs.uniform(-1, 1, (3, 8, 3)) * 0.1).astype(np.float32)
    obj, mode = rs.randint(0, 3, B).astype(np.int32), rs.randint(0, 2, B).astype(np.int32)
    Tg = rand_pose(rs, B)
    Tp = near_pose(rs, Tg, 0.3, 0.03)
    got = run(Tp, Tg, obj, mode, table, n_points)
    norm, xyz = got['norm_avg'].double().cpu().numpy(), got['xyz_avg'].double().cpu().numpy()
    # float64 yardstick, all pairs at once (the padded rows of an object are masked)
    p = table[obj].astype(np.float64)
    valid = np.arange(8)[None, :] < n_points[obj][:, None]
    q = np.einsum('bij,bpj->bpi', Tp[:, :3, :3].astype(np.float64), p) + Tp[:, None, :3, 3]
    g = np.einsum('bij,bpj->bpi', Tg[:, :3, :3].astype(np.float64), p) + Tg[:, None, :3, 3]
    d = g[:, :, None, :] - q[:, None, :, :]                         # (B, gt, pred, 3)
    dist = np.sqrt((d * d).sum(-1))
    dist_s = np.where(valid[:, None, :], dist, np.inf)
    nearest = dist_s.min(2)
    own = np.sqrt(((g - q) ** 2).sum(-1))
    per_point = np.where(mode[:, None] == 1, nearest, own)
    want = (per_point * valid).sum(1) / n_points[obj]
    E = 5 * U * 2.2                                                 # |R p| + |t| < 0.18 + 1.53 + ... < 2.2 here
    tol = 2 * np.sqrt(3) * E + DERIVED_ULPS * U * want
    print('B=70000: worst |norm_avg - ref64| / bound', (np.abs(norm - want) / tol).max())
    assert np.all(np.abs(norm - want) <= tol)
    # the dists_add route on two stretches of pairs of the 8-point object (its batch limit is 65 535, and it takes one P per call)
    from cosypose_amd import distances
    worst = 0.
    for sym in (0, 1):
        ids = np.flatnonzero((obj == 0) & (mode == sym))
        for part in (ids[:100], ids[-100:]):
            fn = distances.dists_add_symmetric if sym else distances.dists_add
            dd = fn(dev(Tp[part]), dev(Tg[part]), dev(table[obj[part]])).double()
            wn, wx = dd.norm(dim=-1).mean(-1).cpu().numpy(), dd.abs().mean(-2).cpu().numpy()
            worst = max(worst, ulps(norm[part], wn).max(), ulps(xyz[part], wx).max())
    print('B=70000: worst deviation from the dists_add route', worst, 'u')
    assert worst <= DERIVED_ULPS
    assert ids[-1] > 65535


def test_nan_pose_and_ids_out_of_range_touch_their_own_row_only():
    Tp, Tg, obj, mode, table, n_points = mixed_batch(seed=13, B=12)
    tab = dev(table)
    clean = run(Tp, Tg, obj, mode, tab, n_points)
    Tp2, obj2 = Tp.copy(), obj.copy()
    Tp2[3, 0, 3] = np.nan                                            # a NaN translation
    Tp2[5, 1, 1] = np.nan                                            # a NaN rotation entry
    obj2[8], obj2[9] = len(n_points), -1                             # rows outside the table: nothing is read
    got = run(Tp2, Tg, obj2, mode, tab, n_points)
    for b in range(12):
        for k in pc.ERROR_FIELDS:
            if b in (3, 5):
                assert torch.isnan(got['norm_avg'][b]) and torch.isnan(got['xyz_avg'][b]).any()
            elif b in (8, 9):
                assert torch.isnan(got['norm_avg'][b]) and torch.isnan(got['xyz_avg'][b]).all()
                assert torch.equal(got['TCO_norm'][b], clean['TCO_norm'][b])
            else:
                assert torch.equal(got[k][b], clean[k][b]), (b, k)
    # n_points beyond the table is clamped to it, a negative one gives the mean of nothing
    n2 = n_points.copy(); n2[0] = -5
    got = run(Tp, Tg, obj, mode, tab, n2)
    assert torch.isnan(got['norm_avg'][torch.from_numpy(obj == 0).cuda()]).all()
    assert torch.equal(got['norm_avg'][torch.from_numpy(obj != 0).cuda()], clean['norm_avg'][torch.from_numpy(obj != 0).cuda()])
    full = run(Tp, Tg, obj, mode, tab, np.full_like(n_points, table.shape[1]))
    over = run(Tp, Tg, obj, mode, tab, np.full_like(n_points, 10 ** 6))
    assert torch.equal(full['norm_avg'], over['norm_avg'])


def test_argument_checks_by_return_code():
    from cosypose_amd._lib import lib, ptr
    l = lib()
    B, n_obj, n_max = 4, 2, 1500
    T, ids, pts, out = torch.eye(4).repeat(B, 1, 1).cuda(), torch.zeros(B, dtype=torch.int32).cuda(), torch.zeros(n_obj, n_max, 3).cuda(), torch.full((B, 8), 7.0).cuda()
    n_pts = torch.full((n_obj,), n_max, dtype=torch.int32).cuda()
    need = l.cosy_pose_errors_workspace_bytes(B, n_max)
    ws = torch.zeros(need + 16, dtype=torch.uint8).cuda()
    args = lambda **kw: [kw.get(k, v) for k, v in dict(p=ptr(T), g=ptr(T), o=ptr(ids), m=ptr(ids), t=ptr(pts), n=ptr(n_pts), B=B, n_obj=n_obj, n_max=n_max,
                                                       e=ptr(out), w=ptr(ws), wb=need, s=None).items()]
    assert l.cosy_pose_errors(*args()) == 0
    for bad in (dict(B=-1), dict(n_obj=0), dict(n_max=0), dict(p=None), dict(g=None), dict(o=None), dict(m=None), dict(t=None), dict(n=None),
                dict(e=None), dict(w=None), dict(wb=need - 1), dict(w=ptr(ws) + 4)):
        out.fill_(7.0)
        assert l.cosy_pose_errors(*args(**bad)) == -1, bad
        torch.cuda.synchronize()
        assert (out == 7.0).all(), bad                                # refused before any launch
    assert l.cosy_pose_errors(*args(B=0, p=None, g=None, o=None, m=None, t=None, n=None, e=None, w=None, wb=0)) == 0


# ---- the meter end to end ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def g():
    return pc.load()


def field_tol(g, field):
    return max(DERIVED_ULPS * U, 2 * float(g[f'dev/{field}'][0]))


def make_mesh_db(g):
    from cosypose_amd.mesh_db import BatchedMeshes
    labels, pts, infos = pc.meshes(g)
    sym = torch.eye(4).reshape(1, 1, 4, 4).repeat(len(labels), 1, 1, 1)
    return labels, BatchedMeshes(infos, labels, torch.from_numpy(pts), sym).cuda().float()


@pytest.mark.parametrize('name', list(pc.CONFIGS))
def test_meter_end_to_end(g, name):
    from cosypose_amd import PoseErrorMeter, PandasTensorCollection
    labels, mesh_db = make_mesh_db(g)
    meter = PoseErrorMeter(mesh_db, **pc.meter_kwargs(g, labels, name))
    for a, scene_id in enumerate(g['scene_ids']):
        gt_infos, gt_poses, pred_infos, pred_poses = pc.frames(g, labels, scene_id)
        pred, gt = PandasTensorCollection(pred_infos, poses=dev(pred_poses)), PandasTensorCollection(gt_infos, poses=dev(gt_poses))
        assert meter.is_data_valid(pred)
        meter.add(pred, gt)
        last = meter.last_candidates
        pc.check_candidates(g, name, a, last['cand_infos'], last['kept'])
        for k in pc.ERROR_FIELDS:
            got, want = last['errors'][k].astype(np.float64), g[f'{name}/{a}/err_{k}'].astype(np.float64)
            rel = np.abs(got - want) / np.maximum(np.abs(want), 1e-30)
            print(f'{name} add {a} {k}: worst deviation from the reference (float32) {rel.max():.3g}, bound {field_tol(g, k):.3g}')
            assert got.shape == want.shape and np.all(rel <= field_tol(g, k)), k
        got, want = pc.check_tables(g, name, a, last['cand_infos'], meter.datas['matches_df'][a], meter.datas['gt_df'][a], meter.datas['pred_df'][a])
        fin = np.isfinite(want)
        assert np.all(np.abs(got[fin] - want[fin]) <= field_tol(g, 'norm_avg') * want[fin])
        assert np.array_equal(np.stack(list(meter.datas['pred_df'][a]['TXO_pred'])), pred_poses[g[f'{name}/{a}/keep_ids']])
    summary, dfs = meter.summary()
    print(name, {k: v for k, v in summary.items() if np.ndim(v) == 0})
    rel = dict(norm=field_tol(g, 'norm_avg'), xyz=field_tol(g, 'xyz_avg'), TCO_xyz=field_tol(g, 'TCO_xyz'), TCO_norm=field_tol(g, 'TCO_norm'))
    pc.check_summary(g, name, summary, lambda k: rel.get(k, 1e-12), lambda k: field_tol(g, 'norm_avg') if k.startswith('AUC') else 0.)
    assert set(dfs) >= {'gt', 'matches', 'preds', 'ap'} and all(isinstance(dfs[k], pd.DataFrame) for k in ('gt', 'matches', 'preds'))
    meter.reset()
    assert len(meter.datas['gt_df']) == 0
