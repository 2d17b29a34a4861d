"""BOP pose errors on the GPU (cosypose_amd/bop_errors.py, csrc/kernels_bop.hip) and BopScoreMeter end to end, against the numpy twins
of tests/bop_ref.py.  The contract is DESIGN.md section 15 (the published definitions restated; not a recording of the BOP toolkit).

Yardsticks (every test prints its figures before it asserts):
  (A) the depth windows pasted into zero frames are torch.equal to HipBatchRenderer.render(..., render_depth=True);
  (B) vsd_counts are np.array_equal to the float32 twin on those depths;
  (C) vsd_counts lie in the float64 twin's [lo, hi] intervals, EPS from the roundings of the distance formula (bop_ref's docstring);
      undecided pixels are at most 0.5 % of the union pixels of the case set, and none on a hand case;
  (D) MSSD / MSPD within the bounds derived in bop_ref.mssd_mspd64_batch of the float64 twin;
  (E) equal bits from run to run, alone or inside a batch, under a tight workspace cap; empty batch; argument checks;
  (F) BopScoreMeter on a seeded two-scene case equals the twin's scores exactly.
"""
import numpy as np
import pandas as pd
import pytest
import torch

import bop_ref as br

pytestmark = pytest.mark.gpu

DELTA = 0.015


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def make_models(n_lat, n_lon, n_obj=3, seed=3, symmetries=None):
    from cosypose_amd import BopModels, synthetic as syn
    verts, faces, colors = syn.make_render_meshes(seed, n_obj, n_lat, n_lon)
    labels = [f'obj_{n + 1:06d}' for n in range(n_obj)]
    return BopModels(labels, verts, faces, symmetries=symmetries, colors_list=colors).cuda()


def full_frames(models, obj, view, TCO, K, hw):
    """(N,H,W) numpy depth of every (object, pose) alone in its view: the package's full-frame render"""
    from cosypose_amd import HipBatchRenderer
    if len(obj) == 0:
        return np.zeros((0,) + tuple(hw), np.float32)
    infos = [dict(name=models.labels[o]) for o in obj]
    _, depth = HipBatchRenderer(models.meshes).render(infos, dev(TCO), dev(K[np.asarray(view)]), resolution=hw, render_depth=True)
    return depth.cpu().numpy()


def windows_as_frames(models, obj, view, TCO, K, hw):
    """boxes (N,4) numpy and the depth windows pasted into zero frames (N,H,W) device tensor"""
    from cosypose_amd import bop_errors as be
    H, W = hw
    T, o, v, Kd = dev(TCO), dev(np.asarray(obj, np.int32)), dev(np.asarray(view, np.int32)), dev(K)
    boxes = be.instance_boxes(T, o, v, Kd, models, hw)
    bx = boxes.cpu().numpy().astype(np.int64)
    size = np.maximum(bx[:, 2] - bx[:, 0] + 1, 0) * np.maximum(bx[:, 3] - bx[:, 1] + 1, 0)
    off = np.where(size > 0, np.cumsum(size) - size, -1)
    store = be.render_windows(T, o, v, Kd, models, hw, boxes, dev(off), int(size.sum()))
    frames = torch.zeros(len(obj), H, W, device='cuda')
    for n in range(len(obj)):
        if size[n]:
            x0, y0, x1, y1 = bx[n]
            assert 0 <= x0 <= x1 < W and 0 <= y0 <= y1 < H, bx[n]
            frames[n, y0:y1 + 1, x0:x1 + 1] = store[off[n]:off[n] + size[n]].view(y1 - y0 + 1, x1 - x0 + 1)
    return bx, size, frames


def pose_at(K, u, v, z, R=None):
    """a pose whose origin projects to pixel coordinate (u, v) at depth z"""
    T = np.eye(4, dtype=np.float64)
    if R is not None:
        T[:3, :3] = R
    T[:3, 3] = [(u - K[0, 2]) * z / K[0, 0], (v - K[1, 2]) * z / K[1, 1], z]
    return T.astype(np.float32)


# ---- (A) windows against the full-frame render ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hw,mesh', [((48, 64), (6, 8)), ((96, 128), (24, 32)), ((37, 53), (12, 16))])
def test_windows_hold_the_bits_of_the_full_frame_render(hw, mesh):
    H, W = hw
    models = make_models(*mesh)
    K = br.make_K(2, H, W)
    K[1, 0, 2] += 3.25; K[1, 1, 1] *= 1.1                                       # a second, different view
    rs = np.random.RandomState(H)
    R = br.rand_pose(rs, 12)[:, :3, :3]
    k0 = K[0]
    z = 0.9
    poses = [
        pose_at(k0, W / 2, H / 2, z, R[0]),                                     # inside the frame
        pose_at(k0, 1.0, H / 2, z, R[1]), pose_at(k0, W - 1.0, H / 2, z, R[2]),  # cut by the left / right edge
        pose_at(k0, W / 2, 0.5, z, R[3]), pose_at(k0, W / 2, H - 1.0, z, R[4]),  # cut by the top / bottom edge
        pose_at(k0, -0.2, -0.3, z, R[5]),                                       # cut by a corner
        pose_at(k0, 40.0 * W, H / 2, z, R[6]),                                  # wholly outside: empty window
        pose_at(k0, 0.0, 0.0, 100.0, R[7]),                                     # a far, tiny object at the corner: a 1-pixel window
        pose_at(k0, W / 2, H / 2, 0.02, R[8]),                                  # across the near plane 0.01
        pose_at(k0, W / 2, H / 2, z, R[9]),                                     # NaN pose (below)
        pose_at(K[1], W / 3, H / 3, 0.7, R[10]),                                # the other view
        pose_at(k0, W / 2, H / 2, 0.25, R[11]),                                 # close to the camera
        pose_at(k0, 0.5, 0.5, 100.0, R[7]),                                     # the tiny object on the centre of pixel (0, 0): one pixel drawn
    ]
    poses[9][0, 3] = np.nan
    TCO = np.stack(poses)
    obj = np.arange(len(poses)) % len(models.labels)
    view = np.zeros(len(poses), np.int64); view[10] = 1
    bx, size, frames = windows_as_frames(models, obj, view, TCO, K, hw)
    want = full_frames(models, obj, view, TCO, K, hw)
    print('boxes', bx.tolist(), 'pixels drawn', (want > 0).sum((1, 2)).tolist())
    assert torch.equal(frames, torch.from_numpy(want).cuda())
    assert size[6] == 0 and size[9] == 0 and not want[6].any() and not want[9].any()
    # A box is floor(u_min - 0.5) .. ceil(u_max - 0.5): one pixel wide only where the frame's edge clips it, and then u_max <= 0.5 -- the
    # centre of that pixel is outside the object, the window holds background.  The smallest window that is drawn into is 2 x 2 around
    # one covered pixel centre.
    assert bx[7].tolist() == [0, 0, 0, 0] and not want[7].any()
    assert bx[12].tolist() == [0, 0, 1, 1] and (want[12] > 0).sum() == 1 and want[12][0, 0] > 99.0
    assert size[0] > 0 and (want[0] > 0).any() and size[0] < H * W              # a window, not the frame
    for n in (1, 2, 3, 4, 5):
        assert (want[n] > 0).any(), n
    assert bx[1][0] == 0 and bx[2][2] == W - 1 and bx[3][1] == 0 and bx[4][3] == H - 1 and bx[5][:2].tolist() == [0, 0]
    z8 = models.meshes.verts[obj[8], :int(models.n_verts[obj[8]])].cpu().numpy().astype(np.float64) @ TCO[8, 2, :3] + TCO[8, 2, 3]
    assert z8.min() < 0.01 < z8.max() and (want[8] > 0).any() and (want[11] > 0).any()
    # every drawn pixel lies inside its box
    for n in range(len(poses)):
        ys, xs = np.nonzero(want[n])
        if len(ys):
            assert bx[n][0] <= xs.min() and xs.max() <= bx[n][2] and bx[n][1] <= ys.min() and ys.max() <= bx[n][3], n


# ---- (B), (C) counts against the float32 and float64 twins ------------------------------------------------------------------------------
def run_counts(models, Tp, Tg, obj, view, K, depth, taus, cap=None):
    from cosypose_amd import bop_errors
    out = bop_errors(dev(Tp), dev(Tg), np.asarray(obj, np.int32), np.asarray(view, np.int32), dev(K), dev(depth), models, taus=taus, delta=DELTA,
                     max_workspace_bytes=cap)
    torch.cuda.synchronize()
    return out


def check_counts(tag, models, Tp, Tg, obj, view, K, depth, taus, tally, hand=False):
    """one bop_errors call against both twins on the package's own full-frame renders -> counts (numpy)"""
    from cosypose_amd.bop_errors import absolute_taus
    hw = depth.shape[1:]
    out = run_counts(models, Tp, Tg, obj, view, K, depth, taus)
    got = out['vsd_counts'].cpu().numpy()
    taus_abs = absolute_taus(taus, obj, models.diameters)
    D_est, D_gt = full_frames(models, obj, view, Tp, K, hw), full_frames(models, obj, view, Tg, K, hw)
    assert got.shape == (len(obj), 2 + taus_abs.shape[1]) and got.dtype == np.int32
    for b in range(len(obj)):
        want = br.vsd_counts32(D_est[b], D_gt[b], depth[view[b]], K[view[b]], taus_abs[b], DELTA)
        lo, hi, undecided, union = br.vsd_intervals64(D_est[b], D_gt[b], depth[view[b]], K[view[b]], taus_abs[b], DELTA)
        tally['undecided'] += undecided; tally['union'] += union; tally['pairs'] += 1
        print(f'{tag} pair {b}: counts {got[b].tolist()} twin32 {want.tolist()} undecided {undecided} of |U| {union}')
        assert np.array_equal(got[b], want), (tag, b)
        assert np.all(lo <= got[b]) and np.all(got[b] <= hi), (tag, b)
        if hand:
            assert undecided == 0
    assert np.array_equal(out['vsd'].cpu().numpy(), br.vsd_from_counts(got)) and out['vsd'].dtype == torch.float64
    return got


def scene_depth(D_gt, rs, wall=2.0, noise=0.004):
    """a measured depth frame: the nearest ground truth, a wall behind, millimetre noise, a few missing pixels and an occluding bar"""
    d = np.where(D_gt > 0, D_gt, np.inf).min(0)
    d = np.where(np.isfinite(d), d, wall).astype(np.float32)
    d = (d + rs.uniform(-noise, noise, d.shape)).astype(np.float32)
    d[rs.uniform(size=d.shape) < 0.03] = 0.0
    d[:, d.shape[1] // 2 - 2:d.shape[1] // 2 + 1] = 0.45
    return d


@pytest.fixture(scope='module')
def tally():
    t = dict(undecided=0, union=0, pairs=0)
    yield t
    print(f'(C) undecided pixels: {t["undecided"]} of {t["union"]} union pixels = {100.0 * t["undecided"] / max(t["union"], 1):.4f} % over {t["pairs"]} pairs')


SCENE_CASES = [((48, 64), (6, 8), 1), ((96, 128), (24, 32), 10), ((37, 53), (12, 16), 16)]


def scene_cases(hw, mesh, n_tau, tally):
    H, W = hw
    models = make_models(*mesh)
    K = br.make_K(2, H, W)
    K[1, 0, 2] -= 2.5
    rs = np.random.RandomState(n_tau)
    R = br.rand_pose(rs, 8)[:, :3, :3]
    c = (W / 2, H / 2)
    Tg = np.stack([pose_at(K[0], 0.2 * W, c[1], 1.2, R[0]), pose_at(K[0], c[0], c[1], 0.8, R[1]), pose_at(K[0], c[0], c[1], 0.9, R[2]),
                   pose_at(K[1], c[0], c[1], 0.7, R[3]), pose_at(K[1], c[0] + 3, c[1] - 2, 0.8, R[4]), pose_at(K[0], c[0], c[1], 0.8, R[5])])
    Tp = np.stack([pose_at(K[0], 0.8 * W, c[1], 1.2, R[0]),                      # disjoint windows (radius < 0.15 fx / 1.2 < 0.3 W)
                   pose_at(K[0], c[0], c[1], 1.6, R[1]),                         # nested: the estimate is twice as far, inside the ground truth's box
                   pose_at(K[0], c[0] + 6, c[1], 0.91, R[2]),                    # half-overlapping
                   br.near_pose(rs, Tg[3:4], 0.05, 0.004)[0],                    # close: most thresholds contested
                   br.near_pose(rs, Tg[4:5], 0.2, 0.01)[0],
                   pose_at(K[0], 40.0 * W, c[1], 0.8, R[5])])                    # the estimate outside the frame: its window is empty
    obj = np.array([0, 1, 2, 0, 1, 2])
    view = np.array([0, 0, 0, 1, 1, 0])
    taus = np.linspace(0.05, 0.5, n_tau) if n_tau > 1 else [0.2]
    D_gt = full_frames(models, obj, view, Tg, K, hw)
    depth = np.stack([scene_depth(D_gt[view == v], rs) for v in (0, 1)])
    got = check_counts(f'{H}x{W} scene', models, Tp, Tg, obj, view, K, depth, taus, tally)
    assert got[0, 1] == 0 and got[5, 1] == 0 and got[:5, 0].min() > 0           # disjoint / empty estimate: nothing in the intersection
    # D_test all missing, and all in front of the object
    zero = check_counts(f'{H}x{W} no depth', models, Tp, Tg, obj, view, K, np.zeros_like(depth), taus, tally)
    assert zero[:5, 0].min() > 0
    front = check_counts(f'{H}x{W} all in front', models, Tp, Tg, obj, view, K, np.full_like(depth, 0.2), taus, tally)
    assert not front.any()
    assert np.array_equal(run_counts(models, Tp, Tg, obj, view, K, np.full_like(depth, 0.2), taus)['vsd'].cpu().numpy(), np.ones((6, len(taus))))


@pytest.mark.parametrize('hw,mesh,n_tau', SCENE_CASES)
def test_counts_equal_the_float32_twin_and_lie_in_the_float64_intervals(hw, mesh, n_tau, tally):
    scene_cases(hw, mesh, n_tau, tally)


def square_models():
    """one fronto-parallel square of 0.08 m (16 pixels at z = 1 under HAND_K), two triangles"""
    from cosypose_amd import BopModels
    v = np.array([[-0.04, -0.04, 0], [0.04, -0.04, 0], [0.04, 0.04, 0], [-0.04, 0.04, 0]], np.float32)
    return BopModels(['square'], [v], [np.array([[0, 1, 2], [0, 2, 3]], np.int32)], diameters=[1.0]).cuda()


def square_pose(u, v, z):
    """the square scaled by z and moved to depth z: it covers the same 16 x 16 pixels around (u, v) at every depth"""
    T = pose_at(br.HAND_K, u, v, z).astype(np.float64)
    T[:3, :3] *= z
    return T.astype(np.float32)


def test_hand_cases_on_the_device(tally):
    """the hand values of the float64 twin (tests/test_bop_errors_host.py), now through the kernels: squares at z = 1, delta = 0.015"""
    models = square_models()
    K = br.HAND_K[None]
    gt, far = square_pose(24.0, 24.0, 1.0), square_pose(5000.0, 24.0, 1.0)
    est = {'same pose': gt, 'moved back 1 cm': square_pose(24.0, 24.0, 1.01), 'moved back 3 cm': square_pose(24.0, 24.0, 1.03),
           'shifted, background missing': square_pose(32.0, 24.0, 1.0), 'shifted, far wall': square_pose(32.0, 24.0, 1.0),
           'shifted, occluder': square_pose(32.0, 24.0, 1.0), 'nothing visible': far}
    for name, _, D_gt, D_test, taus, want in br.hand_cases():
        Tg = far if name == 'nothing visible' else gt
        rendered = full_frames(models, [0], [0], Tg[None], K, br.HAND_HW)[0]
        assert np.array_equal(rendered > 0, D_gt > 0) and np.all(np.abs(rendered[rendered > 0] - 1.0) < 1e-6)      # the mesh draws the hand case's square
        got = check_counts(name, models, est[name][None], Tg[None], [0], [0], K, D_test[None], [taus], tally, hand=True)
        e = br.vsd_from_counts(got)[0, 0]
        print(name, 'e =', e, 'hand value', want)
        assert abs(e - want) < 1e-15


def test_undecided_share_of_the_case_set(tally):
    """(C) must not turn vacuous: runs after the count tests of this module and reads their tally"""
    if tally['pairs'] < 7 + 9 * 6:          # run on its own: the case set is worked off here
        tally = dict(undecided=0, union=0, pairs=0)
        for case in SCENE_CASES:
            scene_cases(*case, tally)
        test_hand_cases_on_the_device(tally)
    share = tally['undecided'] / max(tally['union'], 1)
    print(f'undecided {tally["undecided"]} of {tally["union"]} union pixels: {100 * share:.4f} % ({tally["pairs"]} pairs)')
    assert tally['pairs'] >= 7 + 9 * 6 and tally['union'] > 5000
    assert share <= 0.005


# ---- (D) MSSD and MSPD against the float64 twin ---------------------------------------------------------------------------------------------
TILE, CHUNK = 1024, 8              # BOP_TILE, BOP_CH of kernels_bop.hip
DIST_OBJECTS = [(1, 1), (63, 2), (64, CHUNK - 1), (65, CHUNK), (TILE - 1, CHUNK + 1), (TILE, 64), (TILE + 1, 1), (2 * TILE + 452, CHUNK + 1), (300, 64)]


@pytest.fixture(scope='module')
def dist_models():
    """objects of V vertices and S symmetries (turns about z, the identity first), one per entry of DIST_OBJECTS; the padded rows of the
    vertex table lie far away: a read past n_verts would show"""
    from cosypose_amd import BopModels
    rs = np.random.RandomState(17)
    verts = [(rs.uniform(-1, 1, (V, 3)) * rs.uniform(0.03, 0.12, 3)).astype(np.float32) for V, _ in DIST_OBJECTS]
    faces = [np.zeros((1, 3), np.int32) for _ in DIST_OBJECTS]
    syms = [np.stack([br.rot_z(2 * np.pi * k / S) for k in range(S)]) for _, S in DIST_OBJECTS]
    for s in syms:
        s[0] = np.eye(4)
    models = BopModels([f'o{n}' for n in range(len(verts))], verts, faces, symmetries=syms)
    for n, v in enumerate(verts):
        models.meshes.verts[n, len(v):] = 1e3
        models.sym_table[n, len(syms[n]):] = 1e3
    return models.cuda(), verts, [s.astype(np.float32) for s in syms]


def run_dist(models, Tp, Tg, obj, view, K):
    from cosypose_amd import bop_errors as be
    mssd, mspd = be.mssd_mspd(dev(Tp), dev(Tg), dev(np.asarray(obj, np.int32)), dev(np.asarray(view, np.int32)), dev(K), models)
    torch.cuda.synchronize()
    return mssd.cpu().numpy().astype(np.float64), mspd.cpu().numpy().astype(np.float64)


def check_dist(tag, got, want):
    mssd, mspd = got
    ref3, ref2, b3, b2 = want
    r3, r2 = np.abs(mssd - ref3) / b3, np.abs(mspd - ref2) / b2
    print(f'{tag}: worst |mssd - ref64| / bound {r3.max():.3f}, |mspd - ref64| / bound {r2.max():.3f} (mssd {ref3.min():.4g}..{ref3.max():.4g} m, '
          f'mspd {ref2.min():.4g}..{ref2.max():.4g} px)')
    assert np.all(np.isfinite(b2)) and np.all(r3 <= 1) and np.all(r2 <= 1)
    return max(r3.max(), r2.max())


def dist_pairs(rs, n):
    Tg = br.rand_pose(rs, n)
    Tp = np.concatenate([br.rand_pose(rs, n - n // 2), br.near_pose(rs, Tg[n - n // 2:], 0.1, 0.01)])       # far from and near the ground truth
    return Tp, Tg


@pytest.mark.parametrize('o', range(len(DIST_OBJECTS)), ids=[f'V{V}-S{S}' for V, S in DIST_OBJECTS])
def test_mssd_mspd_shapes(dist_models, o):
    models, verts, syms = dist_models
    rs = np.random.RandomState(o)
    Tp, Tg = dist_pairs(rs, 4)
    K = br.make_K(2, 480, 640); K[1, 0, 0] *= 0.9
    view = np.array([0, 1, 0, 1])
    got = run_dist(models, Tp, Tg, [o] * 4, view, K)
    check_dist(f'V={DIST_OBJECTS[o][0]} S={DIST_OBJECTS[o][1]}', got, br.mssd_mspd64_batch(Tp, Tg, K[view], verts[o], syms[o]))
    # the identity estimate of a listed symmetry: exactly 0 for the half turn (exact in float32) where S is even
    if DIST_OBJECTS[o][1] % 2 == 0:
        half = br.rot_z(np.pi).round().astype(np.float32)
        mssd, mspd = run_dist(models, (Tg[:1].astype(np.float64) @ half).astype(np.float32), Tg[:1], [o], [0], K)
        assert mssd[0] <= 9 * br.U * 3 and mspd[0] <= 1e-2, (mssd, mspd)


def tilt_about(point, angle):
    """a turn by `angle` about an axis through the origin at right angles to `point` (and to z): it moves `point` by angle |point|"""
    axis = np.cross(point.astype(np.float64), [0, 0, 1.0]); axis /= np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    D = np.eye(4); D[:3, :3] = np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)
    return D


@pytest.mark.parametrize('o', range(len(DIST_OBJECTS)), ids=[f'V{V}-S{S}' for V, S in DIST_OBJECTS])
def test_mssd_mspd_tail_vertex_and_last_symmetry_decide(dist_models, o):
    """The result hangs on the LAST vertex (index V - 1: the tail of the last tile) and on the LAST symmetry (the tail of the last chunk):
    the estimate is the ground truth turned by the last symmetry and tilted a little, and the object's outermost vertex -- three times as far out as any
    other -- is moved to the end.  A second object does the same with the FIRST vertex of the last tile.  Dropping either vertex, or
    the last symmetry, moves the float64 value by far more than the bound, so an off-by-one in a tail fails here."""
    from cosypose_amd import BopModels
    _, verts, syms = dist_models
    V, S = DIST_OBJECTS[o]
    rs = np.random.RandomState(100 + o)
    far = np.array([0.4, 0.35, 0.3], np.float32)
    ends = sorted({V - 1, (V - 1) // TILE * TILE})
    objs = []
    for at in ends:
        v = verts[o].copy()
        v[at] = far
        objs.append(v)
    models = BopModels([f'e{n}' for n in range(len(objs))], objs, [np.zeros((1, 3), np.int32)] * len(objs), symmetries=[syms[o]] * len(objs)).cuda()
    K = br.make_K(1, 480, 640)
    Tg = br.rand_pose(rs, len(objs))
    Tp = (Tg.astype(np.float64) @ syms[o][-1].astype(np.float64) @ tilt_about(far, 0.05)).astype(np.float32)
    got = run_dist(models, Tp, Tg, np.arange(len(objs)), np.zeros(len(objs), np.int64), K)
    for n, at in enumerate(ends):
        full = br.mssd_mspd64_batch(Tp[n:n + 1], Tg[n:n + 1], K, objs[n], syms[o])
        check_dist(f'V={V} S={S} extreme vertex at {at}', (got[0][n:n + 1], got[1][n:n + 1]), full)
        without_vertex = br.mssd_mspd64_batch(Tp[n:n + 1], Tg[n:n + 1], K, np.delete(objs[n], at, 0), syms[o]) if V > 1 else None
        without_sym = br.mssd_mspd64_batch(Tp[n:n + 1], Tg[n:n + 1], K, objs[n], syms[o][:-1]) if S > 1 else None
        for name, other in (('vertex', without_vertex), ('symmetry', without_sym)):
            if other is not None:
                print(f'  without the {name}: mssd {other[0][0]:.6g} against {full[0][0]:.6g}, mspd {other[1][0]:.6g} against {full[1][0]:.6g}')
                assert abs(other[0][0] - full[0][0]) > 100 * full[2][0] and abs(other[1][0] - full[1][0]) > 100 * full[3][0], name


def test_mssd_mspd_mixed_objects_in_one_call(dist_models):
    models, verts, syms = dist_models
    rs = np.random.RandomState(23)
    B = 45
    obj = rs.randint(0, len(DIST_OBJECTS), B)
    Tp, Tg = dist_pairs(rs, B)
    K = br.make_K(3, 480, 640); K[2, 1, 2] += 11
    view = rs.randint(0, 3, B)
    got = run_dist(models, Tp, Tg, obj, view, K)
    worst = 0.
    for o in np.unique(obj):
        sel = obj == o
        worst = max(worst, check_dist(f'mixed, object {o}', (got[0][sel], got[1][sel]), br.mssd_mspd64_batch(Tp[sel], Tg[sel], K[view[sel]], verts[o], syms[o])))
    print('mixed: worst ratio to the bound', worst)


def test_mssd_mspd_batch_beyond_a_grid_dimension():
    """70 000 pairs of tiny meshes"""
    from cosypose_amd import BopModels
    B, rs = 70000, np.random.RandomState(5)
    sizes = [(8, 1), (5, 2), (3, 3)]
    verts = [(rs.uniform(-1, 1, (V, 3)) * 0.1).astype(np.float32) for V, _ in sizes]
    syms = [np.stack([np.eye(4)] + [br.rot_z(2 * np.pi * k / S) for k in range(1, S)]) for _, S in sizes]
    models = BopModels(['a', 'b', 'c'], verts, [np.zeros((1, 3), np.int32)] * 3, symmetries=syms).cuda()
    obj = rs.randint(0, 3, B)
    Tg = br.rand_pose(rs, B)
    Tp = br.near_pose(rs, Tg, 0.3, 0.03)
    K = br.make_K(1, 480, 640)
    got = run_dist(models, Tp, Tg, obj, np.zeros(B, np.int64), K)
    for o in range(3):
        sel = obj == o
        check_dist(f'B=70000, object {o}', (got[0][sel], got[1][sel]),
                   br.mssd_mspd64_batch(Tp[sel], Tg[sel], np.repeat(K, sel.sum(), 0), verts[o], syms[o].astype(np.float32)))
    assert np.flatnonzero(obj == 0)[-1] > 65535


# ---- (E) determinism and edge inputs ----------------------------------------------------------------------------------------------------------
def mixed_case(seed=31, B=14, hw=(48, 64)):
    H, W = hw
    half = br.rot_z(np.pi).round()
    models = make_models(6, 8, symmetries=[None, np.stack([np.eye(4), half]), np.stack([br.rot_z(2 * np.pi * k / 9) for k in range(9)]).round(7) * 1.0])
    rs = np.random.RandomState(seed)
    K = br.make_K(2, H, W)
    view = np.arange(B) % 2
    obj = rs.randint(0, 3, B)
    Tg = np.stack([pose_at(K[v], rs.uniform(0.2, 0.8) * W, rs.uniform(0.2, 0.8) * H, rs.uniform(0.7, 1.2), br.rand_pose(rs, 1)[0, :3, :3]) for v in view])
    Tp = br.near_pose(rs, Tg, 0.2, 0.01)
    if B > 7:
        Tp[5] = Tp[2]; Tg[5] = Tg[2]; obj[5] = obj[2]; view[5] = view[2]     # a pair twice, and a ground truth shared by two estimates
        Tg[7] = Tg[3]; obj[7] = obj[3]; view[7] = view[3]
    D_gt = full_frames(models, obj, view, Tg, K, hw)
    depth = np.stack([scene_depth(D_gt[view == v], rs) if (view == v).any() else np.zeros(hw, np.float32) for v in (0, 1)])
    return models, Tp, Tg, obj, view, K, depth


def same(a, b):
    return all(torch.equal(a[k], b[k]) for k in ('mssd', 'mspd', 'vsd_counts', 'vsd'))


def test_two_runs_alone_in_a_batch_and_under_a_tight_cap_give_equal_bits():
    from cosypose_amd import bop_errors as be
    models, Tp, Tg, obj, view, K, depth = mixed_case()
    taus = be.VSD_TAUS
    a, b = run_counts(models, Tp, Tg, obj, view, K, depth, taus), run_counts(models, Tp, Tg, obj, view, K, depth, taus)
    assert same(a, b)
    assert a['vsd_counts'][:, 0].max() > 0 and torch.equal(a['vsd_counts'][5], a['vsd_counts'][2]) and a['mssd'][5] == a['mssd'][2]
    for i in (0, 3, 7, len(obj) - 1):
        alone = run_counts(models, Tp[i:i + 1], Tg[i:i + 1], obj[i:i + 1], view[i:i + 1], K, depth, taus)
        for k in ('mssd', 'mspd', 'vsd_counts', 'vsd'):
            assert torch.equal(alone[k][0], a[k][i]), (i, k)
    perm = np.random.RandomState(0).permutation(len(obj))
    c = run_counts(models, Tp[perm], Tg[perm], obj[perm], view[perm], K, depth, taus)
    for k in ('mssd', 'mspd', 'vsd_counts', 'vsd'):
        assert torch.equal(c[k], a[k][torch.from_numpy(perm).cuda()]), k
    # the tightest cap that still holds every single pair: several chunks, the same counts
    T, o, v, est, gt = be.unique_instances(dev(Tp), dev(Tg), dev(obj.astype(np.int32)), dev(view.astype(np.int32)))
    assert len(T) == 2 * len(obj) - 3                                               # the repeated pair's two instances and the shared ground truth
    bx = be.instance_boxes(T, o, v, dev(K), models, depth.shape[1:]).cpu().numpy().astype(np.int64)
    size = np.maximum(bx[:, 2] - bx[:, 0] + 1, 0) * np.maximum(bx[:, 3] - bx[:, 1] + 1, 0)
    est, gt = est.cpu().numpy(), gt.cpu().numpy()
    cap = int(max(size[e] + (size[g] if g != e else 0) for e, g in zip(est, gt))) * 4
    chunks = be.plan_windows(bx, est, gt, cap // 4)
    print('cap', cap, 'bytes:', len(chunks), 'chunks of', [c['n_pixels'] for c in chunks], 'pixels; unlimited:', int(size.sum()))
    assert len(chunks) >= 3
    assert same(run_counts(models, Tp, Tg, obj, view, K, depth, taus, cap=cap), a)
    with pytest.raises(ValueError, match='alone needs'):
        run_counts(models, Tp, Tg, obj, view, K, depth, taus, cap=cap - 4)


def test_empty_batch_nan_pose_and_ids_out_of_range():
    from cosypose_amd import bop_errors as be
    models, Tp, Tg, obj, view, K, depth = mixed_case(seed=32, B=6)
    out = run_counts(models, Tp[:0], Tg[:0], obj[:0], view[:0], K, depth, be.VSD_TAUS)
    assert out['mssd'].shape == (0,) and out['mspd'].shape == (0,) and out['vsd_counts'].shape == (0, 12) and out['vsd'].shape == (0, 10) and out['mssd'].is_cuda
    clean = run_counts(models, Tp, Tg, obj, view, K, depth, be.VSD_TAUS)
    assert torch.isfinite(clean['mssd']).all() and torch.isfinite(clean['mspd']).all()
    Tp2, Tg2 = Tp.copy(), Tg.copy()
    Tp2[1, 0, 3] = np.nan
    Tg2[4, 1, 1] = np.inf
    got = run_counts(models, Tp2, Tg2, obj, view, K, depth, be.VSD_TAUS)
    for b in range(6):
        if b in (1, 4):
            assert torch.isnan(got['mssd'][b]) and torch.isnan(got['mspd'][b]) and not got['vsd_counts'][b].any() and (got['vsd'][b] == 1).all()
        else:
            for k in ('mssd', 'mspd', 'vsd_counts', 'vsd'):
                assert torch.equal(got[k][b], clean[k][b]), (b, k)
    K2 = K.copy(); K2[1, 0, 0] = np.nan                                              # a non-finite K: every pair of that view
    got = run_counts(models, Tp, Tg, obj, view, K2, depth, be.VSD_TAUS)
    bad = torch.from_numpy(view == 1).cuda()
    assert bad.any() and torch.isnan(got['mssd'][bad]).all() and not got['vsd_counts'][bad].any() and torch.equal(got['mssd'][~bad], clean['mssd'][~bad])
    # the call refuses ids outside its tables on the host ...
    for o2, v2 in ((np.where(np.arange(6) == 2, 3, obj), view), (np.where(np.arange(6) == 2, -1, obj), view), (obj, np.where(np.arange(6) == 0, 2, view))):
        with pytest.raises(ValueError, match='outside'):
            run_counts(models, Tp, Tg, o2, v2, K, depth, be.VSD_TAUS)
    # ... and if such an id reaches the device it reads nothing: NaN and zero counts for its pair alone
    obj2, view2 = obj.astype(np.int32).copy(), view.astype(np.int32).copy()
    obj2[0], obj2[2], view2[3] = 3, -1, 2
    mssd, mspd = be.mssd_mspd(dev(Tp), dev(Tg), dev(obj2), dev(view2), dev(K), models)
    taus_abs = dev(be.absolute_taus(be.VSD_TAUS, obj, models.diameters))
    counts = be.vsd_counts(dev(Tp), dev(Tg), dev(obj2), dev(view2), dev(K), dev(depth), models, taus_abs, DELTA)
    torch.cuda.synchronize()
    for b in range(6):
        if b in (0, 2, 3):
            assert torch.isnan(mssd[b]) and torch.isnan(mspd[b]) and not counts[b].any()
        else:
            assert torch.equal(mssd[b], clean['mssd'][b]) and torch.equal(counts[b], clean['vsd_counts'][b])


def test_argument_checks_leave_the_outputs_untouched():
    from cosypose_amd._lib import lib, ptr
    from cosypose_amd import bop_errors as be
    models, Tp, Tg, obj, view, K, depth = mixed_case(seed=33, B=4)
    l = lib()
    m = models.meshes
    T1, T2, o, v, Kd = dev(Tp), dev(Tg), dev(obj.astype(np.int32)), dev(view.astype(np.int32)), dev(K)
    out = torch.full((2, 4), 7.0).cuda()
    S = models.sym_table.shape[1]
    need = l.cosy_bop_mssd_mspd_workspace_bytes(4, S)
    ws = torch.zeros(need + 16, dtype=torch.uint8).cuda()
    args = lambda **kw: [kw.get(k, val) for k, val in dict(p=ptr(T1), g=ptr(T2), o=ptr(o), v=ptr(v), K=ptr(Kd), x=ptr(m.verts), nv=ptr(models.n_verts),
                                                          s=ptr(models.sym_table), ns=ptr(models.n_sym), B=4, n_obj=3, n_views=2, V=m.verts.shape[1], S=S,
                                                          e3=ptr(out[0]), e2=ptr(out[1]), ws=ptr(ws), wb=need, st=None).items()]
    for bad in (dict(B=-1), dict(n_obj=0), dict(p=None), dict(K=None), dict(e2=None), dict(ws=None), dict(wb=need - 1), dict(ws=ptr(ws) + 4)):
        assert l.cosy_bop_mssd_mspd(*args(**bad)) == -1, bad
        torch.cuda.synchronize()
        assert (out == 7.0).all(), bad
    assert l.cosy_bop_mssd_mspd(*args()) == 0
    torch.cuda.synchronize()
    want = be.mssd_mspd(T1, T2, o, v, Kd, models)
    assert torch.equal(out[0], want[0]) and torch.equal(out[1], want[1])
    # n_tau beyond 16 is refused by the wrapper and by the library
    with pytest.raises(AssertionError):
        run_counts(models, Tp, Tg, obj, view, K, depth, np.linspace(0.01, 0.5, 17))


# ---- (F) the meter end to end -------------------------------------------------------------------------------------------------------------------
def test_meter_end_to_end_equals_the_twin_scores():
    from cosypose_amd import BopScoreMeter, HipSceneRenderer, PandasTensorCollection
    from cosypose_amd.pose_meters import prepare_candidates
    from cosypose_amd.bop_errors import absolute_taus, VSD_TAUS, VSD_THRESHOLDS, MSSD_THRESHOLDS, MSPD_THRESHOLDS
    case = br.e2e_case()
    labels = case['labels']
    half = br.rot_z(np.pi).round()
    models = make_models(12, 16, n_obj=len(labels), seed=9, symmetries=[None, np.stack([np.eye(4), half]), None,
                                                                          np.stack([br.rot_z(np.pi * k / 2).round() for k in range(4)])])
    assert list(models.labels) == labels
    H, W = br.E2E_HW
    meter = BopScoreMeter(models)
    scene_renderer = HipSceneRenderer(models.meshes)
    cand_all, vsd_all, mssd_all, mspd_all, diam_all, n_valid, group_label = [], [], [], [], [], {}, {}
    margins = []
    for scene_id, s in case['scenes'].items():
        names = np.asarray(labels)
        gt_infos = pd.DataFrame(dict(scene_id=s['gt']['scene_id'], view_id=s['gt']['view_id'], label=names[s['gt']['label']], visib_fract=s['gt']['visib_fract']))
        pred_infos = pd.DataFrame(dict(scene_id=s['pred']['scene_id'], view_id=s['pred']['view_id'], label=names[s['pred']['label']], score=s['pred']['score']))
        cam_infos = pd.DataFrame(dict(scene_id=s['cameras']['scene_id'], view_id=s['cameras']['view_id']))
        K = s['cameras']['K']
        # the measured depth: every ground-truth instance of the view in one z-buffer
        depth = scene_renderer.render(gt_infos['label'].values, s['gt']['view_id'], dev(s['gt']['poses']), dev(K), (H, W), render_depth=True)['depth']
        assert (depth > 0).any()
        meter.add(PandasTensorCollection(pred_infos, poses=dev(s['pred']['poses'])), PandasTensorCollection(gt_infos, poses=dev(s['gt']['poses'])),
                  PandasTensorCollection(cam_infos, K=dev(K)), depth)
        # the twin's errors of the same tentative pairs, on the package's full-frame renders
        prep = prepare_candidates(pred_infos, gt_infos, visib_gt_min=0.1)
        cand = prep['cand_infos']
        assert len(cand) >= 6
        pred_poses = s['pred']['poses'][prep['keep_ids']][prep['filtered_ids']][cand['pred_id'].values]
        gt_poses = s['gt']['poses'][cand['gt_id'].values]
        obj = np.array([models.label_to_id[l] for l in cand['label']])
        view = cand['view_id'].values.astype(np.int64)                                # cameras are in view order
        D_est, D_gt = full_frames(models, obj, view, pred_poses, K, (H, W)), full_frames(models, obj, view, gt_poses, K, (H, W))
        taus_abs = absolute_taus(VSD_TAUS, obj, models.diameters)
        depth_h = depth.cpu().numpy()
        sym = models.sym_table.cpu().numpy()
        for n in range(len(cand)):
            counts = br.vsd_counts32(D_est[n], D_gt[n], depth_h[view[n]], K[view[n]], taus_abs[n], DELTA)
            vsd_all.append(br.vsd_from_counts(counts))
            o = obj[n]
            e3, e2, b3, b2 = br.mssd_mspd64_batch(pred_poses[n][None], gt_poses[n][None], K[view[n]][None], models.meshes.verts[o, :int(models.n_verts[o])].cpu().numpy(),
                                                  sym[o, :int(models.n_sym[o])])
            mssd_all.append(e3[0]); mspd_all.append(e2[0]); diam_all.append(models.diameters[o])
            margins.append(min(np.abs(e3[0] - np.asarray(MSSD_THRESHOLDS) * models.diameters[o]).min() / b3[0],
                               np.abs(e2[0] - np.asarray(MSPD_THRESHOLDS) * (W / 640.0)).min() / b2[0]))
            key = (scene_id, int(cand['view_id'][n]), cand['label'][n])
            cand_all.append((key, (scene_id, int(cand['pred_id'][n])), (scene_id, int(cand['gt_id'][n])), float(cand['score'][n])))
        valid = prep['gt_infos'][prep['gt_infos']['valid'].values.astype(bool)]
        for key, rows in valid.groupby(['scene_id', 'view_id', 'label']):
            n_valid[(int(key[0]), int(key[1]), key[2])] = len(rows)
            group_label[(int(key[0]), int(key[1]), key[2])] = key[2]
    print('tentative pairs', len(cand_all), 'groups', len(n_valid), 'smallest distance of an MSSD / MSPD error from a threshold, in bounds:', min(margins))
    assert min(margins) > 1          # no float32 rounding can move an error across a threshold: the scores are then exact
    want = br.bop_scores(cand_all, None, n_valid, group_label, np.stack(vsd_all), mssd_all, mspd_all, diam_all, W,
                         th_vsd=VSD_THRESHOLDS, th_mssd=MSSD_THRESHOLDS, th_mspd=MSPD_THRESHOLDS)
    summary, dfs = meter.summary()
    # an add without a tentative pair (its only prediction has a label without ground truth): its ground truth joins the denominator
    lone = BopScoreMeter(models)
    s = case['scenes'][br.E2E_SCENES[0]]
    gt_infos = pd.DataFrame(dict(scene_id=[77, 77], view_id=[0, 0], label=labels[:2], visib_fract=[0.9, 0.8]))
    pred_infos = pd.DataFrame(dict(scene_id=[77], view_id=[0], label=labels[2:3], score=[0.5]))
    lone.add(PandasTensorCollection(pred_infos, poses=dev(s['pred']['poses'][:1])), PandasTensorCollection(gt_infos, poses=dev(s['gt']['poses'][:2])),
             PandasTensorCollection(pd.DataFrame(dict(scene_id=[77], view_id=[0])), K=dev(s['cameras']['K'][:1])), torch.ones(1, H, W, device='cuda'))
    assert len(lone.last_candidates['cand_infos']) == 0
    empty_summary, _ = lone.summary()
    assert empty_summary['n_gt_valid'] == 2 and empty_summary['AR'] == 0.0 and empty_summary['n_pred'] == 1
    print({k: v for k, v in summary.items() if '/' not in k}, want['all'])
    for k in ('AR', 'AR_VSD', 'AR_MSSD', 'AR_MSPD', 'n_gt_valid'):
        assert summary[k] == want['all'][k], (k, summary[k], want['all'][k])
        for label in sorted(set(group_label.values())):
            if k != 'n_gt_valid':
                assert summary[f'{k}/objects/{label}'] == want[label][k], (k, label)
    assert 0.0 < summary['AR'] < 1.0 and 0.0 < summary['AR_VSD'] < 1.0 and 0.0 < summary['AR_MSSD'] < 1.0 and 0.0 < summary['AR_MSPD'] < 1.0
    assert summary['n_gt_valid'] < summary['n_gt'] and summary['n_pred'] > 0
