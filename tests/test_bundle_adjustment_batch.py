"""Batched bundle adjustment on the GPU (bundle_adjustment.solve_problems, the cosy_ba_batch_* entries of csrc/kernels_ba.hip):
bit identity with MultiviewRefinement.solve per problem, independence of the batch's composition, a NaN neighbour, the reference's
stored runs as batches of one, the decision step on crafted control records, the contract, and predict_scene_states.

All problems are sub-problems of ONE synthetic.make_ba_scene scene (ba_batch_case.sub_scene) on one mesh table, which carries a fifth
mesh without a symmetry for the NaN problem.  Every test prints its figures before it asserts (pytest -s shows them)."""
import math
import pathlib

import numpy as np
import pytest
import torch

import ba_batch_case as bc

pytestmark = pytest.mark.gpu

HERE = pathlib.Path(__file__).resolve().parent
SEED, N_OBJECTS, N_VIEWS = 164, 12, 8
N_ITER = 12
# (views, objects) of the batch; the first is the full scene, the second and the last have ONE candidate (n = 18)
SUBSETS = [(tuple(range(8)), tuple(range(12))), ((2,), (1,)), ((0, 3), (0, 2, 4)), ((1, 2, 4, 6), (5, 3, 1, 0, 7)), ((0, 1, 2, 3, 4), (2, 4, 6, 8, 10, 11)),
           ((5,), (3,))]


def scene_of(P):
    from cosypose_amd import synthetic as syn
    return bc.with_nan_mesh(syn.make_ba_scene(SEED, N_OBJECTS, N_VIEWS, P))


def visible_subsets(scene):
    """SUBSETS restricted to what the scene's visibility offers: a subset without a candidate falls back to its first view's first object"""
    out = []
    for views, objects in SUBSETS:
        sub = bc.sub_scene(scene, views, objects)
        if len(sub['cand_view_id']) == 0:
            v = views[0]
            o = int(np.searchsorted(np.unique(scene['cand_obj_id']), scene['cand_obj_id'][scene['cand_view_id'] == scene['cam_view_id'][v]][0]))
            views, objects = (v,), (o,)
        out.append((views, objects))
    return out


class Case:
    """the batch of one P: the shared mesh_db, a factory of fresh problems and the single path's results per camera mode (computed once)"""

    def __init__(self, P):
        self.scene = scene_of(P)
        self.mesh_db = bc.mesh_db_of(self.scene, device='cuda')
        self.subsets = visible_subsets(self.scene)
        self._single = {}

    def problems(self, subsets=None):
        return [bc.problem_on(bc.sub_scene(self.scene, v, o), self.mesh_db, device='cuda') for v, o in (subsets or self.subsets)]

    def nan_problem(self):
        return bc.problem_on(bc.nan_scene(bc.sub_scene(self.scene, (0, 1, 2), (0, 1, 2, 3))), self.mesh_db, device='cuda')

    def single(self, optimize_cameras):
        """MultiviewRefinement.solve of every problem (the history) and, from a second run of its two steps, the final 9-D states"""
        if optimize_cameras not in self._single:
            res = []
            for p in self.problems():
                out = p.solve(n_iterations=N_ITER, optimize_cameras=optimize_cameras)
                a, c, _ = p.optimize_lm(*p.robust_initialization_TWO_TCW(), n_iterations=N_ITER, optimize_cameras=optimize_cameras)
                res.append(dict(history=out['history'], TWO_9d=a, TCW_9d=c))
            self._single[optimize_cameras] = res
        return self._single[optimize_cameras]


_cases = {}


def case(P):
    if P not in _cases:
        _cases[P] = Case(P)
    return _cases[P]


def assert_same_bits(got, want, tag=''):
    """a solve_problems dict against solve's history + final states (or another solve_problems dict)"""
    hg, hw = got['history'], want['history']
    assert hg['iteration'] == hw['iteration'], (tag, hg['iteration'], hw['iteration'])
    assert hg['lambda'] == hw['lambda'], (tag, hg['lambda'], hw['lambda'])
    for k in ('loss', 'TWO_9d', 'TCW_9d'):
        assert len(hg[k]) == len(hw[k]) == len(hw['iteration']), (tag, k)
        for n, (x, y) in enumerate(zip(hg[k], hw[k])):
            # torch.equal is false for NaN == NaN: the NaN problem's losses are compared as bit patterns
            assert torch.equal(x.reshape(-1).view(torch.int64), y.reshape(-1).view(torch.int64)), (tag, k, n, x, y)
    assert torch.equal(got['TWO_9d'], want['TWO_9d']) and torch.equal(got['TCW_9d'], want['TCW_9d']), tag


def rejected(h):
    return any(b > a for a, b in zip(h['lambda'], h['lambda'][1:]))


def ran_out(h):
    """N_ITER entries and lambda still changing before the last one: the iteration before it decided (it did not set `done`)"""
    return len(h['iteration']) == N_ITER and h['lambda'][-1] != h['lambda'][-2]


@pytest.mark.parametrize('P,optimize_cameras,preconditions', [(31, True, True), (31, False, True), (128, True, False), (129, False, False)])
def test_a_bit_identity_with_the_single_path(P, optimize_cameras, preconditions):
    """Six sub-problems of make_ba_scene(164, 12, 8, P) -- the full scene (n = 180), two with ONE candidate (n = 18), three in between
    -- in one solve_problems call against MultiviewRefinement.solve of each: the iteration and lambda lists, every loss, TWO_9d and
    TCW_9d entry and the final 9-D states are equal bit for bit, with free and with fixed cameras, at P = 31 (one pass of 256 rows),
    128 (exactly one) and 129 (two).  At P = 31 the single path's own results are first checked for what makes the comparison
    non-trivial: at least two history lengths, a problem with a rejected step, one that stops by `done` and one that runs out of its
    12 iterations.  Seed and subsets were picked on an MI355X, where the single path gives at P = 31: free cameras 12, 2, 4, 12, 5, 2
    history entries (the full scene and the 4-view problem reject steps and run out; the others stop by `done`), fixed cameras 12, 2,
    12, 12, 12, 2 (four problems reject steps, three run out)."""
    from cosypose_amd.bundle_adjustment import solve_problems
    c = case(P)
    want = c.single(optimize_cameras)
    hists = [w['history'] for w in want]
    figs = dict(P=P, optimize_cameras=optimize_cameras, n=[9 * (p.n_objects + p.n_views) for p in c.problems()], candidates=[p.n_candidates for p in c.problems()],
                entries=[len(h['iteration']) for h in hists], rejected=[rejected(h) for h in hists], ran_out=[ran_out(h) for h in hists])
    print('FIGURE batch bit identity', figs)
    assert figs['n'][0] == 180 and 18 in figs['n'] and 1 in figs['candidates']
    if preconditions:
        assert len(set(figs['entries'])) >= 2 and any(figs['rejected']) and any(figs['ran_out'])
        assert any(len(h['iteration']) < N_ITER for h in hists)                        # left the loop early: `done`
    got = solve_problems(c.problems(), n_iterations=N_ITER, optimize_cameras=optimize_cameras)
    assert len(got) == len(want)
    for g, (a, b) in enumerate(zip(got, want)):
        assert_same_bits(a, b, f'problem {g}')
    if not optimize_cameras:
        assert all(torch.equal(t, h['TCW_9d'][0]) for h in (o['history'] for o in got) for t in h['TCW_9d'])


@pytest.mark.parametrize('optimize_cameras', [True, False])
def test_b_composition_independence(optimize_cameras):
    """the same problems reversed, each alone (G = 1), and with one of them twice: every problem keeps its bits"""
    from cosypose_amd.bundle_adjustment import solve_problems
    c = case(31)
    kw = dict(n_iterations=N_ITER, optimize_cameras=optimize_cameras)
    base = solve_problems(c.problems(), **kw)
    rev = solve_problems(c.problems()[::-1], **kw)[::-1]
    alone = [solve_problems([p], **kw)[0] for p in c.problems()]
    order = [0, 3, 1, 3, 2, 4, 5, 3]
    dup = solve_problems(c.problems([c.subsets[i] for i in order]), **kw)
    for g, b in enumerate(base):
        assert_same_bits(rev[g], b, f'reversed {g}')
        assert_same_bits(alone[g], b, f'alone {g}')
    for i, d in zip(order, dup):
        assert_same_bits(d, base[i], f'duplicated {i}')


def test_c_nan_neighbour():
    """A problem whose candidates name a mesh with n_sym = 0 (loss NaN from the first linearisation) in the middle of the batch: its
    lambda history is the single path's -- x 11 per iteration from 1e-3 up to the 1e7 clamp, 12 entries, every step rejected -- and
    every other problem keeps the bits of test (a)."""
    from cosypose_amd.bundle_adjustment import solve_problems
    c = case(31)
    problems = c.problems()
    got = solve_problems(problems[:2] + [c.nan_problem()] + problems[2:], n_iterations=N_ITER)
    nan = got.pop(2)
    single = c.nan_problem().solve(n_iterations=N_ITER)['history']
    lam, want = 1e-3, []
    for _ in range(N_ITER):
        want.append(lam)
        lam = min(lam * 11, 1e7)
    print('FIGURE nan neighbour lambda', nan['history']['lambda'])
    assert nan['history']['lambda'] == single['lambda'] == want and want[-1] == 1e7 and want[-2] == 1e7 and want[-3] < 1e7
    assert nan['history']['iteration'] == single['iteration'] == list(range(N_ITER))
    assert all(bool(torch.isnan(l)) for l in nan['history']['loss']) and all(bool(torch.isnan(l)) for l in single['loss'])
    assert all(torch.equal(t, nan['history']['TWO_9d'][0]) for t in nan['history']['TWO_9d'])          # no step was taken
    assert torch.equal(nan['TWO_9d'], nan['history']['TWO_9d'][0])
    for g, (a, b) in enumerate(zip(got, c.single(True))):
        assert_same_bits(a, b, f'problem {g} beside the NaN problem')


# ---- the reference's stored runs, as batches of one.  The constants are those of tests/test_bundle_adjustment.py (run_and_compare;
# measured in the docstring of its test_solve_vs_reference): loss history relative to the largest loss, the gauge-free
# inv(TWC) TWO per candidate relative to its largest entry, both under the ceiling that separates float64 in another order from a
# single-precision operation ----
SOLVE_CEILING = 1e-6
LOSS_TOL = 1e-6
TCO_TOL = 2.9e-7


def rel_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / np.abs(want).max())


def T_of_pose9d(p):
    """float64 numpy restatement of compute_transform_from_pose9d"""
    p = np.asarray(p, np.float64)
    x = p[..., 0:3] / np.linalg.norm(p[..., 0:3], axis=-1, keepdims=True)
    z = np.cross(x, p[..., 3:6])
    z = z / np.linalg.norm(z, axis=-1, keepdims=True)
    y = np.cross(z, x)
    T = np.zeros(p.shape[:-1] + (4, 4))
    T[..., :3, :3] = np.stack([x, y, z], -1)
    T[..., :3, 3] = p[..., 6:]
    T[..., 3, 3] = 1
    return T


def pose_bound(want, dtype):
    """allowed |got - want| per entry of a 4x4 output: one float32 ulp of max(1, |x|) for float32 candidates, 1e-12 for float64"""
    if dtype == torch.float64:
        return np.full(want.shape, 1e-12)
    return np.spacing(np.maximum(1, np.abs(want)).astype(np.float32)).astype(np.float64)


def check_poses(out, dtype, tag):
    """the four 4x4 outputs against the float64 numpy conversion of the returned 9-D states"""
    h = out['history']
    pairs = [('objects', 'TWO', T_of_pose9d(out['TWO_9d'].cpu().numpy())), ('cameras', 'TWC', np.linalg.inv(T_of_pose9d(out['TCW_9d'].cpu().numpy())))]
    if 'TWO_9d' in h:
        pairs += [('objects_init', 'TWO', T_of_pose9d(h['TWO_9d'][0].cpu().numpy())),
                  ('cameras_init', 'TWC', np.linalg.inv(T_of_pose9d(h['TCW_9d'][0].cpu().numpy())))]
    for key, name, want in pairs:
        got = getattr(out[key], name)
        assert got.dtype == dtype and got.shape == want.shape, (tag, key)
        err = np.abs(got.double().cpu().numpy() - want)
        print(f'FIGURE poses {tag} {key}: max |got - want| {err.max():.3e}')
        assert (err <= pose_bound(want, dtype)).all(), (tag, key, err.max())


@pytest.mark.parametrize('prefix,dtype', [('s1_', torch.float64), ('s2_', torch.float64), ('s3_', torch.float64), ('s4_', torch.float64), ('s5_', torch.float64),
                                          ('f2_', torch.float64), ('f4_', torch.float64), ('s1_', torch.float32)])
def test_d_reference_runs_as_batches_of_one(prefix, dtype):
    """Every stored run of tests/golden/reference_golden_ba.npz through solve_problems([problem]): run_and_compare's assertions (the same
    initialisation to 1e-12, the same iteration list, the lambda history EXACTLY -- every accept / reject / stop decision agrees --,
    loss history and gauge-free TCO within LOSS_TOL / TCO_TOL), the fixed-camera runs never move a camera, and the 4x4 outputs are the
    float64 conversion of the returned 9-D states.  With float32 candidates (s1_) the states differ from the stored float64 run's
    inputs, so only the output dtype and the 4x4 conversion are checked there."""
    from cosypose_amd import synthetic as syn
    from cosypose_amd.bundle_adjustment import MultiviewRefinement, invert_T, solve_problems
    from cosypose_amd.mesh_db import BatchedMeshes
    g = dict(np.load(HERE / 'golden' / 'reference_golden_ba.npz', allow_pickle=False))
    key = prefix + 'in_'
    scene = {k[len(key):]: v for k, v in g.items() if k.startswith(key)}
    p = MultiviewRefinement(*syn.ba_scene_collections(scene, BatchedMeshes, dtype=dtype, device='cuda'))
    fixed = prefix.startswith('f')
    out, = solve_problems([p], sample_n_init=1, **(dict(optimize_cameras=False) if fixed else {}))
    h = out['history']
    check_poses(out, dtype, prefix)
    assert out['n_host_reads'] <= math.ceil(50 / 8) + 1
    assert all(len(h[k]) == len(h['iteration']) for k in ('loss', 'lambda', 'TWO_9d', 'TCW_9d')) and h['TWO_9d'][0].dtype == torch.float64
    if dtype != torch.float64:
        assert torch.isfinite(out['objects'].TWO).all() and h['loss'][-1] < h['loss'][0]
        return
    assert float((out['objects_init'].TWO.cpu() - torch.from_numpy(g[prefix + 'TWO_init'])).abs().max()) <= 1e-12
    assert float((out['cameras_init'].TWC.cpu() - torch.from_numpy(g[prefix + 'TWC_init'])).abs().max()) <= 1e-12
    assert len(h['iteration']) == len(g[prefix + 'hist_iteration']) and h['iteration'] == g[prefix + 'hist_iteration'].tolist()
    assert h['lambda'] == g[prefix + 'hist_lambda'].tolist()                        # exactly: products of the same constants
    TCO = invert_T(out['cameras'].TWC)[p.cand_view_ids] @ out['objects'].TWO[p.cand_obj_ids]     # the gauge-free output
    figs = dict(loss=rel_err(torch.stack(h['loss']).cpu(), g[prefix + 'hist_loss']), TCO=rel_err(TCO.cpu(), g[prefix + 'rel_TCO']))
    print(f'FIGURE batch of one {prefix}', figs, 'entries', len(h['iteration']), 'host reads', out['n_host_reads'])
    assert figs['loss'] < min(LOSS_TOL, SOLVE_CEILING) and figs['TCO'] < min(TCO_TOL, SOLVE_CEILING), figs
    if fixed:
        assert all(torch.equal(t, h['TCW_9d'][0]) for t in h['TCW_9d']) and torch.equal(out['TCW_9d'], h['TCW_9d'][0])
        assert torch.equal(out['cameras'].TWC, out['cameras_init'].TWC) and not torch.equal(out['objects'].TWO, out['objects_init'].TWO)


# ---- the decision step alone ----
EPS, L_DOWN, L_UP = 1e-5, 9., 11.


def loop_body(r, n, rows):
    """the reference's loop body from its appends on (bundle_adjustment.py:251-276 there) on one control record"""
    if r['finished']:
        return
    rows.append((n, r['lambd'], r['loss']))
    r['n_hist'] += 1
    if r['done']:
        r['finished'] = 1               # `break`
        return
    rho = r['loss'] - r['next_loss']
    if abs(rho) < EPS:
        r['done'] = 1
    elif rho > EPS:
        r['loss'] = r['next_loss']
        r['lambd'] = max(r['lambd'] / L_DOWN, 1e-7)
        r['prev_update'] = 1
    else:
        r['lambd'] = min(r['lambd'] * L_UP, 1e7)
        r['prev_update'] = 0


def test_e_decision_step_on_crafted_records():
    """cosy_ba_batch_record + cosy_ba_batch_decide alone, two rounds, on records that cover rho = +-eps exactly, one ulp above and below
    either, 0, NaN, +-inf, inf - inf; lambda at and next to both clamps (and where lambda / 9 and lambda x 11 land on them); `done`
    already set with prev_update 0 and 1; a problem already finished; and the last history row.  Records and history rows are compared
    as bit patterns with the Python restatement above."""
    from cosypose_amd._lib import lib, ptr, stream, check, BaCtrl
    up, down = (lambda v: float(np.nextafter(v, np.inf))), (lambda v: float(np.nextafter(v, -np.inf)))
    inf, nan = float('inf'), float('nan')
    cases = []      # loss, next_loss, lambda, done, prev_update, finished
    for rho in (EPS, up(EPS), down(EPS), 0.5):
        cases += [(rho, 0., 1e-3, 0, 0, 0), (0., rho, 1e-3, 0, 1, 0)]            # rho and -rho, exactly
    cases += [(2.5, 2.5, 1e-3, 0, 1, 0), (nan, 1., 1e-3, 0, 1, 0), (1., nan, 1e-3, 0, 0, 0), (nan, nan, 1e-3, 0, 1, 0), (inf, 1., 1e-3, 0, 0, 0),
              (1., inf, 1e-3, 0, 1, 0), (inf, inf, 1e-3, 0, 1, 0), (-inf, 1., 1e-3, 0, 1, 0), (1., -inf, 1e-3, 0, 0, 0)]
    for lam in (1e-7, up(1e-7), 9e-7, up(9e-7), down(9e-7), 8e-7, 1e7, down(1e7), 1e7 / 11, up(1e7 / 11), down(1e7 / 11), 9.2e5, 5.):
        cases += [(3., 1., lam, 0, 0, 0), (1., 3., lam, 0, 1, 0)]               # accepted and rejected at this lambda
    cases += [(3., 1., 1e-3, 1, 0, 0), (3., 1., 1e-3, 1, 1, 0), (1., 3., 1e-3, 1, 1, 0), (3., 1., 1e-3, 0, 1, 1), (3., 1., 1e-3, 1, 0, 1)]
    G, n_rows, first = len(cases), 7, 5          # rounds at iterations 5 and 6 = the last of 7
    ctrl = np.zeros(G, dtype=np.dtype(BaCtrl))
    for i, (loss, nxt, lam, done, prev, fin) in enumerate(cases):
        ctrl[i] = (loss, nxt, lam, done, prev, fin, first if i % 2 else first - 2)      # the next history row: 5 or 3
    want = [dict(zip(ctrl.dtype.names, rec.tolist())) for rec in ctrl]
    want_rows = [[] for _ in range(G)]
    d_ctrl = torch.from_numpy(ctrl.view(np.uint8).reshape(G, -1).copy()).cuda()
    h_it = torch.full((G, n_rows), -7, dtype=torch.int32, device='cuda')
    h_lam = torch.full((G, n_rows), -7., dtype=torch.float64, device='cuda')
    h_loss = torch.full((G, n_rows), -7., dtype=torch.float64, device='cuda')
    for n in (first, first + 1):
        check(lib().cosy_ba_batch_record(ptr(d_ctrl), G, n, n_rows, None, 0, 0, 0, None, None, ptr(h_it), ptr(h_lam), ptr(h_loss), None, None, stream()))
        check(lib().cosy_ba_batch_decide(ptr(d_ctrl), G, L_DOWN, L_UP, EPS, None, 0, 0, None, None, None, None, stream()))
        for r, rows in zip(want, want_rows):
            loop_body(r, n, rows)
    got = d_ctrl.cpu().numpy().view(ctrl.dtype).ravel()
    bits = lambda v: np.asarray(v, np.float64).view(np.int64)
    h_it, h_lam, h_loss = h_it.cpu().numpy(), h_lam.cpu().numpy(), h_loss.cpu().numpy()
    seen = set()
    for i, (r, rows) in enumerate(zip(want, want_rows)):
        for k in ('loss', 'next_loss', 'lambd'):
            assert bits(got[i][k]) == bits(r[k]), (i, cases[i], k, got[i], r)
        for k in ('done', 'prev_update', 'finished', 'n_hist'):
            assert got[i][k] == r[k], (i, cases[i], k, got[i], r)
        k0 = int(ctrl[i]['n_hist'])
        assert np.array_equal(h_it[i, k0:k0 + len(rows)], [x[0] for x in rows]), (i, cases[i])
        assert np.array_equal(bits(h_lam[i, k0:k0 + len(rows)]), bits([x[1] for x in rows])), (i, cases[i])
        assert np.array_equal(bits(h_loss[i, k0:k0 + len(rows)]), bits([x[2] for x in rows])), (i, cases[i])
        untouched = np.ones(n_rows, bool)
        untouched[k0:k0 + len(rows)] = False
        assert (h_it[i, untouched] == -7).all() and (h_lam[i, untouched] == -7).all() and (h_loss[i, untouched] == -7).all(), (i, cases[i])
        seen.add((r['done'], r['prev_update'], r['finished'], len(rows)))
    assert any(k0 + len(rows) == n_rows for k0, rows in zip(ctrl['n_hist'].tolist(), want_rows))       # the last row was written
    assert len(seen) >= 6 and {len(rows) for rows in want_rows} == {0, 1, 2}


def test_f_contract():
    from cosypose_amd import synthetic as syn
    from cosypose_amd.bundle_adjustment import solve_problems
    c = case(31)
    assert solve_problems([]) == []
    other = syn.make_ba_scene(12, 3, 2, 31)
    with pytest.raises(ValueError, match='mesh_db'):
        solve_problems(c.problems()[:2] + [bc.problem_on(other, bc.mesh_db_of(other, device='cuda'), device='cuda')])
    big_scene = syn.make_ba_scene(3, 122, 8, 8, p_visible=0.2)                # 130 blocks > 128
    big_db = bc.mesh_db_of(big_scene, device='cuda')
    with pytest.raises(ValueError, match='> 128'):
        solve_problems([bc.problem_on(bc.sub_scene(big_scene, (0, 1), (0, 1, 2)), big_db, device='cuda'), bc.problem_on(big_scene, big_db, device='cuda')])
    for n_iter, poll in ((N_ITER, 8), (N_ITER, 1), (N_ITER, 5), (3, 8), (1, 1)):
        out = solve_problems(c.problems(), n_iterations=n_iter, poll_every=poll)
        print('FIGURE host reads', dict(n_iterations=n_iter, poll_every=poll, reads=out[0]['n_host_reads'], launched=out[0]['n_iterations_launched']))
        assert 1 <= out[0]['n_host_reads'] <= math.ceil(n_iter / poll) + 1
        assert all(len(o['history']['iteration']) <= n_iter for o in out)
        if n_iter == N_ITER:      # polling changes when the launches stop, never a result
            for g, (a, b) in enumerate(zip(out, c.single(True))):
                assert_same_bits(a, b, f'poll_every={poll}, problem {g}')
    lean = solve_problems(c.problems(), n_iterations=N_ITER, history=False)
    again = solve_problems(c.problems(), n_iterations=N_ITER)
    for a, b, w in zip(lean, again, c.single(True)):
        assert set(a['history']) == {'iteration', 'lambda', 'loss'} and {'TWO_9d', 'TCW_9d'} <= set(b['history'])
        assert a['history']['iteration'] == w['history']['iteration'] and a['history']['lambda'] == w['history']['lambda']
        assert all(torch.equal(x, y) for x, y in zip(a['history']['loss'], w['history']['loss']))
        assert torch.equal(a['TWO_9d'], w['TWO_9d']) and torch.equal(a['TCW_9d'], w['TCW_9d'])
        assert_same_bits(b, w, 'second run')
        for k, name in (('objects', 'TWO'), ('cameras', 'TWC'), ('objects_init', 'TWO'), ('cameras_init', 'TWC')):
            assert torch.equal(getattr(a[k], name), getattr(b[k], name)), k
    # the early stop: two one-candidate problems are done after their first step, so the launches end at the first poll
    quick = solve_problems(c.problems([c.subsets[1], c.subsets[5]]), n_iterations=50, poll_every=4)
    assert quick[0]['n_iterations_launched'] == 4 and quick[0]['n_host_reads'] == 2 and [len(q['history']['iteration']) for q in quick] == [2, 2]


def split_scene(g):
    """scene 164 of the matching fixture with its views and objects cut into two halves that share nothing: two view groups"""
    import ransac_case as rc
    cand, cams, mesh_db = rc.collections(g, 'c_', 'cuda')
    truth = rc.scene_of(g, 'c_')['cand_obj_id']
    views, objects = np.unique(cand.infos['view_id']), np.unique(truth)
    in_a, obj_a = np.isin(cand.infos['view_id'], views[:len(views) // 2]), np.isin(truth, objects[:len(objects) // 2])
    return cand[np.where(in_a == obj_a)[0]], cams, mesh_db


def test_g_predict_scene_states():
    """Two scenes through predict_scene_states -- scene 164 of the matching fixture, and the same scene cut into two halves without a
    common object, which gives two view groups -- against predict_scene_state of each: the same keys, the same `infos` frames, and
    poses within one float32 ulp of max(1, |x|) (the candidates are float32; the bound of test d)."""
    import ransac_case as rc
    from cosypose_amd.multiview_predictor import MultiviewScenePredictor
    g = rc.load()
    cand, cams, mesh_db = rc.collections(g, 'c_', 'cuda')
    cand2, _, _ = split_scene(g)
    scenes = []
    for scene_id, cnd in ((3, cand), (4, cand2)):
        cm = cams[np.arange(len(cams))]
        cnd.infos['scene_id'], cnd.infos['group_id'] = scene_id, 0
        cm.infos['scene_id'], cm.infos['batch_im_id'] = scene_id, np.arange(len(cm))
        scenes.append((cnd, cm))
    predictor = MultiviewScenePredictor(mesh_db.aabb(), mesh_db)
    got = predictor.predict_scene_states(scenes, ba_n_iter=N_ITER, ba_history=True)
    want = [predictor.predict_scene_state(cnd, cm, ba_n_iter=N_ITER) for cnd, cm in scenes]
    n_groups = [len(set(w['scene/cameras'].infos['view_group'])) for w in want]
    print('FIGURE predict_scene_states view groups', n_groups, 'objects', [len(w['scene/objects']) for w in want])
    assert n_groups == [1, 2] and len(got) == 2
    for a, b in zip(got, want):
        assert set(a) == set(b)
        for k in ('cand_inputs', 'cand_matched', 'scene/objects', 'scene/cameras', 'ba_input', 'ba_output', 'ba_output+all_cand'):
            assert a[k].infos.equals(b[k].infos), k
            assert set(a[k].tensors) == set(b[k].tensors), k
            for name in a[k].tensors:
                x, y = a[k].tensors[name], b[k].tensors[name]
                assert x.dtype == y.dtype and x.shape == y.shape, (k, name)
                err = (x.double() - y.double()).abs().cpu().numpy()
                assert (err <= pose_bound(y.double().cpu().numpy(), torch.float32)).all(), (k, name, err.max())
        assert len(a['ba_history']) == len(b['ba_history'])
        for ha, hb in zip(a['ba_history'], b['ba_history']):
            assert ha['iteration'] == hb['iteration'] and ha['lambda'] == hb['lambda']
            assert all(torch.equal(x, y) for k in ('loss', 'TWO_9d', 'TCW_9d') for x, y in zip(ha[k], hb[k]))
