"""Bundle adjustment on the GPU (cosypose_amd/bundle_adjustment.py, csrc/kernels_ba.hip) against the reference's own float64 runs in
tests/golden/reference_golden_ba.npz / reference_golden_ba_jac.npz (tests/golden/generate_golden_ba.py).

Both sides compute in float64 and differ in operation order only, so the bounds are MEASURED ones: 10 x the worst figure seen on an
MI355X, each written next to its measurement in the docstring of its test -- and, independent of the measurement, a ceiling that
separates "float64, another order" from "a single-precision operation or a wrong term got in" (float32 rounding is 6e-8).  Every test
prints its figures before it asserts (pytest -s shows them).
"""
import ctypes
import pathlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = pathlib.Path(__file__).resolve().parent
LIN_CEILING = 1e-9       # linearisation and normal equations: anything above is not summation order
SOLVE_CEILING = 1e-6     # whole solve: the reference's own float32-vs-float64 figure is 6e-7 ... 1e-3
DIST_TOL = 1e-5          # float32 distances, relative (the convention of test_gpu_parity.py)
THRESHOLD = 25           # optimize_lm's default residuals_threshold


@pytest.fixture(scope='module')
def golden():
    g = dict(np.load(HERE / 'golden' / 'reference_golden_ba.npz', allow_pickle=False))
    g.update(np.load(HERE / 'golden' / 'reference_golden_ba_jac.npz', allow_pickle=False))
    return g


def scene_inputs(g, prefix):
    key = prefix + 'in_'
    return {k[len(key):]: v for k, v in g.items() if k.startswith(key)}


def problem_of(scene, dtype=torch.float64):
    from cosypose_amd import synthetic as syn
    from cosypose_amd.bundle_adjustment import MultiviewRefinement
    from cosypose_amd.mesh_db import BatchedMeshes
    return MultiviewRefinement(*syn.ba_scene_collections(scene, BatchedMeshes, dtype=dtype, device='cuda'))


def rel_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / np.abs(want).max())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


LIN_CASES = [(s, tag) for s in ('s1_', 's2_', 's4_') for tag in ('init', 'final')]
LIN_TOL = 6.4e-13        # 10 x the worst of test_linearise_vs_reference, see its docstring
NE_TOL = 4e-14           # 10 x the worst of test_normal_equations_vs_dense_float64 (A; b at the initial states)
NE_SCALED_TOL = 4.8e-13  # b relative to its un-cancelled scale, all states
NE_SAME_E_TOL = 4e-10    # b against J^T (own e), all states


@pytest.mark.parametrize('prefix,tag', LIN_CASES)
def test_linearise_vs_reference(golden, prefix, tag):
    """errors, loss and the compact Jacobian at the initial and the final state of scenes 1, 2, 4 against the reference's autograd
    Jacobian.  Figure: max |got - want| / max |want| per tensor.  Measured on an MI355X, worst over the six cases: errors 6.4e-14 (scene 1, final
    state; <= 2.0e-14 at the initial states, where max |e| is larger), loss 3.4e-15, J_TWO 4.7e-16, J_TCW 4.4e-16 -> LIN_TOL = 6.4e-13."""
    g = golden
    p = problem_of(scene_inputs(g, prefix))
    errors, loss, J_TWO, J_TCW = p.forward_jacobian(dev(g[f'{prefix}TWO_9d_{tag}']), dev(g[f'{prefix}TCW_9d_{tag}']), THRESHOLD)
    figs = dict(errors=rel_err(errors.cpu(), g[f'{prefix}{tag}_errors']), loss=rel_err(loss.cpu(), g[f'{prefix}{tag}_loss']),
                J_TWO=rel_err(J_TWO.cpu(), g[f'{prefix}{tag}_J_TWO']), J_TCW=rel_err(J_TCW.cpu(), g[f'{prefix}{tag}_J_TCW']))
    print(f'FIGURE linearise {prefix}{tag}', figs)
    assert J_TWO.shape == g[f'{prefix}{tag}_J_TWO'].shape and errors.dtype == torch.float64
    assert max(figs.values()) < min(LIN_TOL, LIN_CEILING), figs


def dense_jacobian(g, prefix, tag):
    J_TWO, J_TCW = g[f'{prefix}{tag}_J_TWO'], g[f'{prefix}{tag}_J_TCW']
    n_obj, n_views = len(g[prefix + 'objinfo_obj_id']), len(g[prefix + 'in_cam_view_id'])
    n_res = J_TWO.shape[0]
    per_cand = n_res // len(g[prefix + 'obj_ids'])
    obj, view = np.repeat(g[prefix + 'obj_ids'], per_cand), np.repeat(g[prefix + 'view_ids'], per_cand)
    J = np.zeros((n_res, 9 * (n_obj + n_views)))
    rows = np.arange(n_res)[:, None]
    J[rows, obj[:, None] * 9 + np.arange(9)] = J_TWO
    J[rows, (n_obj + view[:, None]) * 9 + np.arange(9)] = J_TCW
    return torch.from_numpy(J)


@pytest.mark.parametrize('prefix,tag', LIN_CASES)
def test_normal_equations_vs_dense_float64(golden, prefix, tag):
    """A = J^T J and b = J^T e from the per-candidate blocks against the products formed in torch float64 on the CPU from the
    reference's Jacobian scattered to dense and the reference's stored errors.  Figures, measured on an MI355X:

    A, all six cases, max |got - want| / max |want|: worst 9.9e-16.
    b at the three initial states, the same figure: 3.5e-15, 4.0e-15, 3.0e-15 -> NE_TOL = 4e-14 for both.
    b at all six states relative to max(|J|^T |e|), the scale of b's terms before they cancel: 3.5e-15, 4.0e-15,
        2.8e-15 at the initial and 4.2e-14, 1.8e-14, 4.8e-14 at the final states -> NE_SCALED_TOL = 4.8e-13.
        At a converged state b = J^T e has cancelled to 1e-5 of its terms (max |b| 2.7 ... 7.6 against max(|J|^T |e|) 1.2e5 ... 4.3e5), so
        that the two sides' e -- each correct to the rounding of a pixel coordinate, ~1e-13 px -- move b by 7.2e-10, 2.8e-9, 1.4e-9
        of max |b| at the three final states (printed as b_final_rel_max): the stored b is not determined to 1e-9 of its own largest
        entry there, by the reference's own rounding.  Relative to the un-cancelled scale the comparison with the stored e holds
        at every state, under the same 1e-9 ceiling.
    b against J^T e with the e this linearisation returned (pinned to the stored one by test_linearise_vs_reference), relative to
        max |b|, all six states: worst 3.9e-11 -> NE_SAME_E_TOL.  This isolates the accumulation of the blocks from the rounding of e."""
    g = golden
    p = problem_of(scene_inputs(g, prefix))
    state = dev(g[f'{prefix}TWO_9d_{tag}']), dev(g[f'{prefix}TCW_9d_{tag}'])
    A, b = p.normal_equations(*state, THRESHOLD)
    e_own = p.forward_jacobian(*state, THRESHOLD)[0].cpu()
    J = dense_jacobian(g, prefix, tag)
    e = torch.from_numpy(g[f'{prefix}{tag}_errors'])
    b_ref = J.t() @ e
    scale = float((J.abs().t() @ e.abs()).max())
    figs = dict(A=rel_err(A.cpu(), J.t() @ J), b_scaled=float((b.cpu() - b_ref).abs().max()) / scale, b_same_e=rel_err(b.cpu(), J.t() @ e_own))
    b_rel_max = rel_err(b.cpu(), b_ref)
    print(f'FIGURE normal equations {prefix}{tag}', figs, 'b_init_rel_max' if tag == 'init' else 'b_final_rel_max', b_rel_max,
          'max|b|', float(b_ref.abs().max()), 'scale', scale)
    assert torch.equal(A, A.t())                    # both triangles are the same sums in the same order
    assert figs['A'] < min(NE_TOL, LIN_CEILING), figs
    if tag == 'init':
        assert b_rel_max < min(NE_TOL, LIN_CEILING), b_rel_max
    assert figs['b_scaled'] < min(NE_SCALED_TOL, LIN_CEILING), figs
    assert figs['b_same_e'] < min(NE_SAME_E_TOL, LIN_CEILING), figs


@pytest.mark.parametrize('prefix', ['s2_', 's4_', 's5_'])
@pytest.mark.parametrize('lambd', [1e-7, 1e-3, 1e7])
def test_solve_residual_vs_torch_solve(golden, prefix, lambd):
    """h = (A + lambda I)^-1 b from the Cholesky kernel: the relative residual |(A + lambda I) h - b| / |b|, evaluated in float64 on the
    CPU, is at most max(10 x the same figure of torch.linalg.solve on the CPU, 10 n 2.2e-16).  The residual and not h: at
    lambda = 1e-7 h has few determined digits along the gauge directions.  Measured ratios ours / torch on an MI355X (full-matrix Cholesky, no Schur
    elimination), rows scene 2 / 4 / 5 (n = 90 / 180 / 252): lambda 1e-7: 0.89, 1.11, 1.72; 1e-3: 1.05, 1.52, 1.08; 1e7: 1.14, 2.23, 1.94; every
    residual is between 2.7e-16 and 1.1e-15."""
    g = golden
    p = problem_of(scene_inputs(g, prefix))
    A, b = p.normal_equations(dev(g[prefix + 'TWO_9d_init']), dev(g[prefix + 'TCW_9d_init']), THRESHOLD)
    h = p._solve(lambd).cpu()
    A, b = A.cpu(), b.cpu()
    n = A.shape[0]
    M = A + lambd * torch.eye(n, dtype=torch.float64)
    ours = float(torch.norm(M @ h - b) / torch.norm(b))
    theirs = float(torch.norm(M @ torch.linalg.solve(M, b) - b) / torch.norm(b))
    print(f'FIGURE solve {prefix} lambda={lambd:g} n={n}: residual {ours:.3e}, torch.linalg.solve {theirs:.3e}, ratio {ours / theirs:.2f}')
    assert torch.isfinite(h).all()
    assert ours <= max(10 * theirs, 10 * n * 2.2e-16)


LOSS_TOL = 1e-6          # 10 x the worst of the whole-solve tests would be 3.7e-6: the ceiling binds, see test_solve_vs_reference
TCO_TOL = 2.9e-7         # 10 x the worst of the whole-solve tests (free and fixed cameras)


def run_and_compare(g, prefix, **kwargs):
    from cosypose_amd.bundle_adjustment import invert_T
    p = problem_of(scene_inputs(g, prefix))
    out = p.solve(sample_n_init=1, **kwargs)
    h = out['history']
    assert float((out['objects_init'].TWO.cpu() - torch.from_numpy(g[prefix + 'TWO_init'])).abs().max()) <= 1e-12
    assert float((out['cameras_init'].TWC.cpu() - torch.from_numpy(g[prefix + 'TWC_init'])).abs().max()) <= 1e-12
    assert len(h['iteration']) == len(g[prefix + 'hist_iteration']) and h['iteration'] == g[prefix + 'hist_iteration'].tolist()
    assert h['lambda'] == g[prefix + 'hist_lambda'].tolist()                        # exactly: products of the same constants
    assert all(len(h[k]) == len(h['iteration']) for k in ('loss', 'TWO_9d', 'TCW_9d', 'objects', 'cameras'))
    TCO = invert_T(out['cameras'].TWC)[p.cand_view_ids] @ out['objects'].TWO[p.cand_obj_ids]     # the gauge-free output
    figs = dict(loss=rel_err(torch.stack(h['loss']).cpu(), g[prefix + 'hist_loss']), TCO=rel_err(TCO.cpu(), g[prefix + 'rel_TCO']))
    print(f'FIGURE solve {prefix}', figs, 'entries', len(h['iteration']))
    # the first entry is the initial state (the last one need not be the optimum: a step accepted in the last iteration is not appended)
    assert torch.equal(h['objects'][0].TWO, out['objects_init'].TWO) and torch.equal(h['cameras'][0].TWC, out['cameras_init'].TWC)
    assert figs['loss'] < min(LOSS_TOL, SOLVE_CEILING) and figs['TCO'] < min(TCO_TOL, SOLVE_CEILING), figs
    return p, out


@pytest.mark.parametrize('prefix', ['s1_', 's2_', 's3_', 's4_', 's5_'])
def test_solve_vs_reference(golden, prefix):
    """The whole solve against the reference's float64 run: the same initialisation (<= 1e-12), the same number of history entries, the
    same lambda history exactly (so every accept / reject / stop decision agrees), and the loss history and inv(TWC) TWO per candidate
    within bounds.  TWO / TWC themselves are not compared: the world frame is free.  Measured on an MI355X, scenes 1-5 then the two fixed-camera
    runs: loss history 9.7e-8, 2.9e-7, 1.8e-7, 3.7e-7, 2.3e-7, 5.8e-14, 7.0e-8 (relative to the largest loss; the worst entry is the one
    after the first accepted step); relative TCO 3.4e-9, 1.2e-9, 4.6e-9, 1.1e-9, 1.7e-10, 6.7e-16, 2.9e-8 -> TCO_TOL = 2.9e-7; for the
    loss 10 x the worst would exceed the ceiling, so LOSS_TOL is the ceiling, 1e-6.

    These figures are not this implementation's rounding: the reference run against ITSELF with nothing changed but the order of the
    unknowns in its pseudo-inverse differs from its own stored history by 5.6e-8, 5.4e-8, 1.2e-7, 4.1e-7, 1.7e-7, 1.8e-13, 5.6e-7 on
    the same scenes (generate_golden_ba.py prints and stores them as *_self_loss): cond(A + lambda I) ~ 1e12 amplifies the rounding
    of a step along the weakly determined directions.  The generator refuses a scene on which the reference does not reproduce its
    own history within the ceiling."""
    run_and_compare(golden, prefix)


@pytest.mark.parametrize('prefix', ['f2_', 'f4_'])
def test_solve_fixed_cameras_vs_reference(golden, prefix):
    """optimize_cameras=False on the scenes with exact view pairs (the reference accepts 21 and 10 steps there): the same checks, and
    the cameras never move."""
    p, out = run_and_compare(golden, prefix, optimize_cameras=False)
    h = out['history']
    assert all(torch.equal(t, h['TCW_9d'][0]) for t in h['TCW_9d'])
    assert all(torch.equal(c.TWC, out['cameras_init'].TWC) for c in h['cameras'])
    assert not torch.equal(out['objects'].TWO, out['objects_init'].TWO)


def test_solve_twice_bit_identical(golden):
    g = golden
    outs = [problem_of(scene_inputs(g, 's5_')).solve() for _ in range(2)]
    a, b = outs
    for k in ('objects', 'cameras', 'objects_init', 'cameras_init'):
        for name in a[k].tensors:
            assert torch.equal(a[k].tensors[name], b[k].tensors[name]), (k, name)
    ha, hb = a['history'], b['history']
    assert ha['iteration'] == hb['iteration'] and ha['lambda'] == hb['lambda'] and len(ha['iteration']) >= 4
    for k in ('loss', 'TWO_9d', 'TCW_9d'):
        assert all(torch.equal(x, y) for x, y in zip(ha[k], hb[k])), k
    for x, y in zip(ha['objects'], hb['objects']):
        assert torch.equal(x.TWO, y.TWO)
    for x, y in zip(ha['cameras'], hb['cameras']):
        assert torch.equal(x.TWC, y.TWC)


def test_larger_scene_descends():
    """25 objects, 8 views, 200 points per object, n_iterations=100 as MultiviewScenePredictor calls it (no reference output: a run of
    the reference takes more than a minute on a CPU).  That the loss falls holds for a wrong Jacobian too (a step is accepted only if
    it does), so the loss of EVERY state of the device's own history is also recomputed by tests/ba_ref.py (float64 on the CPU,
    alignment included): this pins the two-pass loss (2P = 400 rows) at the shape bench_ba.py times, without the amplification a
    whole-solve comparison has.  Figure: max |got - want| / max |want| over the history, under LIN_TOL.  Measured on an MI355X:
    1.1e-15 over the 5 entries (smallest symmetry margin 12 px)."""
    import ba_ref
    from cosypose_amd import synthetic as syn
    scene = syn.make_ba_scene(7, 25, 8, 200)
    p = problem_of(scene)
    out = p.solve(n_iterations=100)
    loss = torch.stack(out['history']['loss'])
    print('FIGURE larger scene: candidates', p.n_candidates, 'entries', len(loss), 'loss', float(loss[0]), '->', float(loss[-1]),
          'time_opt', out['time_opt'])
    assert torch.isfinite(loss).all() and (loss[1:] <= loss[:-1]).all() and loss[-1] < loss[0]
    refs = [ba_ref.reference_of_scene(scene, a.cpu().numpy(), c.cpu().numpy(), THRESHOLD, jacobian=False)
            for a, c in zip(out['history']['TWO_9d'], out['history']['TCW_9d'])]
    fig = rel_err(loss.cpu(), [r['loss'] for r in refs])
    print('FIGURE larger scene: loss history against ba_ref', fig, 'smallest symmetry margin', min(float(r['margin'].min()) for r in refs))
    assert len(refs) == len(loss) >= 2 and min(r['margin'].min() for r in refs) >= 1e-3
    assert fig < min(LIN_TOL, LIN_CEILING)
    TWO, TWC = out['objects'].TWO, out['cameras'].TWC
    assert torch.isfinite(TWO).all() and torch.isfinite(TWC).all()
    R = TWO[:, :3, :3]
    assert float((R @ R.transpose(1, 2) - torch.eye(3, dtype=R.dtype, device=R.device)).abs().max()) < 1e-12
    assert float((torch.det(R.cpu()) - 1).abs().max()) < 1e-12


def test_float32_candidates_come_back_float32(golden):
    p = problem_of(scene_inputs(golden, 's1_'), dtype=torch.float32)
    out = p.solve()
    assert out['objects'].TWO.dtype == torch.float32 and out['cameras'].TWC.dtype == torch.float32
    assert out['history']['TWO_9d'][0].dtype == torch.float64           # the states stay float64
    assert torch.isfinite(out['objects'].TWO).all() and out['history']['loss'][-1] < out['history']['loss'][0]


def test_align_vs_reference(golden):
    """distances and the chosen symmetry of every candidate at the initial state (the generator made sure that the best symmetry beats
    the runner-up by >= 1e-3 px)"""
    for prefix in ('s1_', 's2_', 's3_', 's4_', 's5_'):
        g = golden
        p = problem_of(scene_inputs(g, prefix))
        dists, aligned = p.align_TCO_cand(dev(g[prefix + 'TWO_9d_init']), dev(g[prefix + 'TCW_9d_init']))
        assert np.array_equal(p._device_state()['best'].cpu().numpy(), g[prefix + 'align_sym'])
        figs = dict(dists=rel_err(dists.cpu(), g[prefix + 'align_dists']), aligned=rel_err(aligned.cpu(), g[prefix + 'align_TCO']))
        print(f'FIGURE align {prefix}', figs)
        assert max(figs.values()) < LIN_CEILING


def test_symmetric_distance_reprojected_vs_reference(golden):
    from cosypose_amd import symmetric_distances as sd
    from cosypose_amd.mesh_db import BatchedMeshes
    g = golden
    gd = np.load(HERE / 'golden' / 'reference_golden_dist.npz')
    n_obj = gd['sd_pts'].shape[0]
    labels = np.array([f'obj_{i:06d}' for i in range(1, n_obj + 1)])
    infos = {l: dict(label=l, n_sym=int(gd['sd_nsym'][i])) for i, l in enumerate(labels)}
    mesh_db = BatchedMeshes(infos, labels, torch.from_numpy(gd['sd_pts']), torch.from_numpy(gd['sd_sym'])).float().cuda()
    d, S12 = sd.symmetric_distance_reprojected(dev(gd['sd_T1']), dev(gd['sd_T2']), dev(g['sdr_K']), labels[gd['sd_obj']], mesh_db)
    print('FIGURE reprojected distance', rel_err(d.cpu(), g['sdr_dists']))
    assert d.dtype == torch.float32 and rel_err(d.cpu(), g['sdr_dists']) < DIST_TOL
    assert np.array_equal(S12.cpu().numpy(), g['sdr_S12'])
    assert len({tuple(s.ravel()) for s in g['sdr_S12']}) > 2               # non-trivial choices
    d0, S0 = sd.symmetric_distance_reprojected(dev(gd['sd_T1'][:0]), dev(gd['sd_T2'][:0]), dev(g['sdr_K'][:0]), labels[:0], mesh_db)
    assert d0.shape == (0,) and S0.shape == (0, 4, 4)
    # an object id outside the table and an object with n_sym = 0 are marked (NaN, -1, zero S12), the other items are unaffected
    from cosypose_amd._lib import lib, ptr, stream
    B = len(gd['sd_obj'])
    obj = gd['sd_obj'].astype(np.int32).copy(); obj[1] = n_obj; obj[2] = -1
    n_sym = gd['sd_nsym'].astype(np.int32).copy(); n_sym[obj[0]] = 0
    T1, T2, K, pts, sym = dev(gd['sd_T1']), dev(gd['sd_T2']), dev(g['sdr_K']), dev(gd['sd_pts']), dev(gd['sd_sym'])
    d2 = torch.full((B,), 7., device='cuda'); best = torch.full((B,), 7, dtype=torch.int32, device='cuda'); S2 = torch.full((B, 4, 4), 7., device='cuda')
    assert lib().cosy_symmetric_distance_reprojected(ptr(T1), ptr(T2), ptr(K), ptr(dev(obj)), ptr(pts), ptr(sym), ptr(dev(n_sym)), B, n_obj,
                                                     pts.shape[1], sym.shape[1], ptr(d2), ptr(best), ptr(S2), stream()) == 0
    marked = np.isin(np.arange(B), [1, 2]) | (obj == obj[0])
    assert np.array_equal(np.isnan(d2.cpu().numpy()), marked) and np.array_equal(best.cpu().numpy() == -1, marked)
    assert float(S2[torch.from_numpy(marked).cuda()].abs().max()) == 0.
    assert torch.equal(d2[~torch.from_numpy(marked).cuda()], d[~torch.from_numpy(marked).cuda()])


def test_c_abi_contract():
    """argument checks of the new entries, on return codes only: every call here is refused before anything is launched"""
    from cosypose_amd._lib import lib
    l = lib()
    EINVAL, ESIZE = -1, -4
    buf = torch.zeros(4096, dtype=torch.float64, device='cuda')
    P_ = buf.data_ptr()
    ok_ids = (ctypes.c_int * 2)(0, 0)

    def arr(*v):
        return (ctypes.c_int * len(v))(*v)

    def upload(cand_obj, cand_view, cand_mesh, obj_mesh, n_cand=2, n_obj=2, n_views=2, n_mesh=2, ids=P_):
        return l.cosy_ba_upload_ids(ctypes.addressof(cand_obj) if cand_obj else None, ctypes.addressof(cand_view), ctypes.addressof(cand_mesh),
                                    ctypes.addressof(obj_mesh), n_cand, n_obj, n_views, n_mesh, ids, None)
    assert upload(arr(0, 2), ok_ids, ok_ids, ok_ids) == EINVAL and b'object id 2' in l.cosy_last_error()
    assert upload(ok_ids, arr(-1, 0), ok_ids, ok_ids) == EINVAL and b'view id -1' in l.cosy_last_error()
    assert upload(ok_ids, ok_ids, arr(0, 5), ok_ids) == EINVAL and b'mesh id 5' in l.cosy_last_error()
    assert upload(ok_ids, ok_ids, ok_ids, arr(0, 2)) == EINVAL and b'object 1' in l.cosy_last_error()
    assert upload(None, ok_ids, ok_ids, ok_ids) == EINVAL and b'null' in l.cosy_last_error()
    assert upload(ok_ids, ok_ids, ok_ids, ok_ids, n_cand=0) == EINVAL

    def align(n_cand=2, n_obj=2, n_views=2, P=8, S=4, first=P_):
        return l.cosy_ba_align(first, P_, P_, P_, P_, P_, P_, P_, n_cand, n_obj, n_views, 2, P, S, P_, P_, P_, None)

    def linearize(n_cand=2, n_obj=2, n_views=2, P=8, first=P_, ws=P_):
        return l.cosy_ba_linearize(first, P_, P_, P_, P_, P_, n_cand, n_obj, n_views, 2, P, 25.0, P_, P_, P_, P_, None, None, ws, None)
    for fn in (align, linearize):
        assert fn(n_cand=0) == EINVAL and fn(n_cand=-3) == EINVAL and fn(P=0) == EINVAL and fn(n_obj=0) == EINVAL and fn(n_views=0) == EINVAL
        assert fn(first=None) == EINVAL and b'null' in l.cosy_last_error()
        assert fn(n_obj=100, n_views=29) == ESIZE and b'129' in l.cosy_last_error()
    assert linearize(ws=None) == EINVAL and align(S=0) == EINVAL
    assert l.cosy_ba_solve(P_, P_, 18, 0.0, P_, P_, None) == EINVAL and b'lambda' in l.cosy_last_error()
    assert l.cosy_ba_solve(P_, P_, 18, -1e-3, P_, P_, None) == EINVAL
    assert l.cosy_ba_solve(P_, P_, 0, 1e-3, P_, P_, None) == EINVAL
    assert l.cosy_ba_solve(None, P_, 18, 1e-3, P_, P_, None) == EINVAL
    assert l.cosy_ba_solve(P_, P_, 1153, 1e-3, P_, P_, None) == ESIZE and b'1153' in l.cosy_last_error()
    assert l.cosy_ba_workspace_bytes(2, 8, 100, 29) == 0 and l.cosy_ba_workspace_bytes(0, 8, 2, 2) == 0
    n = 9 * 128
    assert l.cosy_ba_workspace_bytes(1000, 200, 100, 28) >= 8 * max(n * n, 1000 * 190)     # linearise and solve share it
    assert l.cosy_ba_workspace_bytes(1000, 200, 2, 2) >= 8 * 1000 * 190
    assert l.cosy_symmetric_distance_reprojected(P_, P_, P_, None, P_, P_, None, 2, 2, 0, 4, P_, P_, P_, None) == EINVAL
    assert l.cosy_symmetric_distance_reprojected(None, P_, P_, None, P_, P_, None, 2, 2, 8, 4, P_, P_, P_, None) == EINVAL
    assert l.cosy_symmetric_distance_reprojected(P_, P_, P_, None, P_, P_, None, 2, 1, 8, 4, P_, P_, P_, None) == EINVAL     # 2 items, 1 table row
    assert l.cosy_symmetric_distance_reprojected(None, None, None, None, None, None, None, 0, 0, 8, 4, None, None, None, None) == 0
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.         # nothing was launched or copied


def test_python_contract(golden):
    from cosypose_amd import synthetic as syn
    from cosypose_amd._lib import CosyHipError
    from cosypose_amd.bundle_adjustment import MultiviewRefinement, SamplerError
    from cosypose_amd.mesh_db import BatchedMeshes
    scene = scene_inputs(golden, 's3_')
    cand, cams, pairs, mesh_db = syn.ba_scene_collections(scene, BatchedMeshes, device='cuda')
    with pytest.raises(ValueError, match='no candidates'):
        MultiviewRefinement(cand[np.arange(0)], cams, pairs, mesh_db)
    with pytest.raises(ValueError, match='view_id'):
        MultiviewRefinement(cand, cams[np.arange(1, len(cams))], pairs, mesh_db)
    lone = scene['cam_view_id'][2]
    keep = np.where((scene['pair_view1'] != lone) & (scene['pair_view2'] != lone))[0]
    with pytest.raises(SamplerError):
        MultiviewRefinement(cand, cams, pairs[keep], mesh_db).solve()
    with pytest.raises(CosyHipError, match='ROCm device only'):       # no CPU fallback
        MultiviewRefinement(*syn.ba_scene_collections(scene, BatchedMeshes)).solve()
    big = syn.make_ba_scene(3, 122, 8, 8, p_visible=0.2)                # 130 blocks > 128
    with pytest.raises(ValueError, match='> 128'):
        problem_of(big).solve()
