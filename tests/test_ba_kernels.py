"""The bundle-adjustment kernels (csrc/kernels_ba.hip: align, linearise, accumulate, the Cholesky solve, the float32 reprojected
symmetric distance) against tests/ba_ref.py -- a plain torch-float64 restatement with an autograd Jacobian, pinned to the reference's
stored runs by tests/test_bundle_adjustment_host.py -- at the shapes where their loops take another trip: more than one 256-row pass
of linearise, more or fewer than 256 points in the symmetry distance, n above 1024 / no multiple of 32 / below 32 in the solve, the
128 x 128 grid of accumulate, and id tables that the Python class cannot produce.

Scenes come from synthetic.make_ba_scene (seeded, nothing stored).  The state is derived from the candidates and perturbed by
N(0, 3e-3) per entry of the 9-D states (ba_ref.state_from_candidates), so that max |e| is a few pixels.

Bounds.  The figures and the constants LIN_CEILING (1e-9, the hard line everywhere), LIN_TOL and DIST_TOL are those of
test_bundle_adjustment.py.  J, aligned, dists, loss: max |got - want| / max |want| < LIN_TOL.  errors: relative to the larger of
max |e| and 1e-3 of the largest pixel coordinate they are differences of.  A and b: relative to the largest entry of their
UN-CANCELLED scales |J|^T |J| and |J|^T |e|, at most (N + 64) 2.2e-16 with N = 2P x the most candidates summed into one block: a sum
of N products is off by at most about N 2^-52 of that scale whatever its order, the 64 covers the rounding already in J and e.
Every test prints its figures before it asserts.
"""
import functools

import numpy as np
import pytest
import torch

import ba_ref
from test_bundle_adjustment import DIST_TOL, LIN_CEILING, LIN_TOL, THRESHOLD, dev, problem_of, rel_err

pytestmark = pytest.mark.gpu

EPS = 2.2e-16
SEED = 11                # scene and perturbation; every candidate's symmetry margin is >= 20 px at every shape below (asserted >= 1e-3)


def sum_bound(terms):
    return (terms + 64) * EPS


def solve_rule(A, b, lambd, h):
    """test_solve_residual_vs_torch_solve's rule -> (our relative residual, torch.linalg.solve's, the bound), float64 on the CPU"""
    n = A.shape[0]
    M = A + lambd * torch.eye(n, dtype=torch.float64)
    ours = float(torch.norm(M @ h - b) / torch.norm(b))
    theirs = float(torch.norm(M @ torch.linalg.solve(M, b) - b) / torch.norm(b))
    return ours, theirs, max(10 * theirs, 10 * n * EPS)


def linearisation_figures(got, ref):
    """got: dict of numpy arrays from the device (best, dists (n_cand), aligned, errors, loss, J_TWO, J_TCW, A, b); ref: ba_ref.reference"""
    nc = len(ref['best'])
    e_scale = max(np.abs(ref['errors']).max(), 1e-3 * ref['pix_scale'])
    return dict(dists=rel_err(got['dists'], ref['dists'][np.arange(nc), ref['best']]), aligned=rel_err(got['aligned'], ref['aligned']),
                errors=float(np.abs(got['errors'] - ref['errors']).max() / e_scale), loss=rel_err(got['loss'], ref['loss']),
                J_TWO=rel_err(got['J_TWO'], ref['J_TWO']), J_TCW=rel_err(got['J_TCW'], ref['J_TCW']),
                A=float(np.abs(got['A'] - ref['A']).max() / ref['A_scale'].max()),
                b=float(np.abs(got['b'] - ref['b']).max() / ref['b_scale'].max()))


def assert_linearisation(tag, got, ref):
    figs = linearisation_figures(got, ref)
    bound = sum_bound(ref['terms'])
    print(f'FIGURE {tag}', {k: f'{v:.2e}' for k, v in figs.items()}, f'(N + 64) eps = {bound:.2e}', 'margin', float(ref['margin'].min()),
          'max|e|', float(np.abs(ref['errors']).max()))
    assert ref['margin'].min() >= 1e-3
    assert np.array_equal(got['best'], ref['best'])
    for k in ('dists', 'aligned', 'errors', 'loss', 'J_TWO', 'J_TCW'):
        assert figs[k] < min(LIN_TOL, LIN_CEILING), (k, figs)
    assert figs['A'] <= min(bound, LIN_CEILING) and figs['b'] <= min(bound, LIN_CEILING), (figs, bound)
    assert np.array_equal(got['A'], got['A'].T)                    # both triangles are the same sums in the same order


def through_the_class(p, state):
    dists, aligned = p.align_TCO_cand(*state)
    best = p._device_state()['best'].clone()
    errors, loss, J_TWO, J_TCW = p.forward_jacobian(*state, THRESHOLD)
    A, b = p.normal_equations(*state, THRESHOLD)
    out = dict(dists=dists, aligned=aligned, best=best, errors=errors, loss=loss, J_TWO=J_TWO, J_TCW=J_TCW, A=A, b=b)
    return {k: v.cpu().numpy() for k, v in out.items()}


def same_bits(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


# ---- a. linearise and align across the 256-row passes --------------------------------------------------------------------------------
PASS_SHAPES = [(1, 1, 1), (2, 2, 31), (2, 2, 127), (2, 2, 128), (2, 2, 129), (3, 2, 200), (2, 2, 257), (2, 2, 1000)]


@pytest.mark.parametrize('n_objects,n_views,P', PASS_SHAPES)
def test_linearise_across_row_passes(n_objects, n_views, P):
    """(objects, views, P) with 2P = 2, 62, 254, 256 (exactly one pass), 258 (a pass and two rows), 400 (bench_ba.py's), 514 and 2000
    (the production table: 8 passes, the last with 208 rows); P also crosses the 256-point stride of the symmetry distance both ways.
    best exactly; dists, aligned, errors, loss, J_TWO, J_TCW, A, b against ba_ref; A == A^T; two calls give equal bits.
    Measured on an MI355X, worst over the eight shapes: dists 4.8e-15, aligned 0 (the same products), errors 2.9e-14,
    loss 6.0e-15, J_TWO 5.2e-16, J_TCW 4.3e-16 (LIN_TOL = 6.4e-13 holds everywhere); A 1.4e-15 and b 7.2e-15 of their un-cancelled
    scales against (N + 64) eps = 1.5e-14 at P = 1 (A 2.7e-16, b 1.7e-16 there) ... 8.9e-13 at P = 1000 (A 7.7e-16, b 6.8e-15)."""
    from cosypose_amd import synthetic as syn
    scene = syn.make_ba_scene(SEED, n_objects, n_views, P)
    state = ba_ref.state_from_candidates(scene, SEED)
    ref = ba_ref.reference_of_scene(scene, *state, THRESHOLD)
    p = problem_of(scene)
    got = through_the_class(p, (dev(state[0]), dev(state[1])))
    assert_linearisation(f'row passes {n_objects, n_views, P}', got, ref)
    assert same_bits(got, through_the_class(p, (dev(state[0]), dev(state[1]))))


# ---- b. the block limit ---------------------------------------------------------------------------------------------------------------
def test_accumulate_and_solve_at_the_block_limit():
    """120 objects + 8 views = 128 blocks (a 128 x 128 grid of accumulate), n = 1152, 195 candidates, P = 8: A, b, loss against ba_ref,
    exact zeros in every object-object and view-view off-diagonal block and every (object, view) block without a candidate, then the
    Cholesky solve at lambda = 1e-3 under the residual rule of test_solve_residual_vs_torch_solve.  Measured on an MI355X: dists 4.8e-15,
    errors 1.2e-14, loss 5.6e-16, J 4.5e-16, A 7.6e-16 and b 2.0e-15 against (N + 64) eps = 1.3e-13 (N = 512: one view holds 32
    candidates); residual of the solve 7.9e-16 against torch.linalg.solve's 3.8e-15."""
    from cosypose_amd import synthetic as syn
    scene = syn.make_ba_scene(3, 120, 8, 8, p_visible=0.2)
    state = ba_ref.state_from_candidates(scene, SEED)
    ref = ba_ref.reference_of_scene(scene, *state, THRESHOLD)
    p = problem_of(scene)
    n_obj, n_views, n_cand = p.n_objects, p.n_views, p.n_candidates
    assert (n_obj + n_views, n_cand, 9 * (n_obj + n_views)) == (128, 195, 1152)
    got = through_the_class(p, (dev(state[0]), dev(state[1])))
    assert_linearisation('block limit', got, ref)
    cand_obj, cand_view, _, _ = ba_ref.scene_ids(scene)
    filled = np.eye(128, dtype=bool)
    filled[cand_obj, n_obj + cand_view] = filled[n_obj + cand_view, cand_obj] = True
    empty = ~np.kron(filled, np.ones((9, 9), dtype=bool))
    assert empty.sum() == 81 * (128 * 128 - 128 - 2 * len(set(zip(cand_obj, cand_view)))) and (got['A'][empty] == 0.).all()
    assert (ref['A'][empty] == 0.).all()
    lambd = 1e-3
    h = p._solve(lambd).cpu()
    ours, theirs, bound = solve_rule(torch.from_numpy(got['A']), torch.from_numpy(got['b']), lambd, h)
    print(f'FIGURE block limit solve n=1152 lambda={lambd:g}: residual {ours:.3e}, torch.linalg.solve {theirs:.3e}, bound {bound:.3e}')
    assert torch.isfinite(h).all()
    assert ours <= bound


# ---- c. id tables that only the C ABI can express ------------------------------------------------------------------------------------
ABI_P, ABI_S, ABI_N_MESH = 129, 5, 6
N_SYM_TABLES = dict(below=(2, 3, 4, 1, 0, 4),        # S larger than every n_sym
                    clamped=(2, 3, 7, 1, 0, 4))      # mesh 2: n_sym > S, clamped to S
ABI_OBJ_MESH = (0, 2)
# three candidates on (object 0, view 0); candidate 3 of object 0 carries ANOTHER mesh than its object's, with another n_sym
ABI_CANDS = dict(obj=(0, 0, 0, 0, 1, 1), view=(0, 0, 0, 1, 0, 1), mesh=(0, 0, 0, 1, 2, 2))
# the symmetry that aligns each candidate (it was made with the inverse): candidate 2's is excluded by its mesh's n_sym = 2 (residuals of tens of pixels, past the
# loss threshold), candidate 4's (the fifth of mesh 2) counts only where n_sym = 7 is clamped to S = 5 and not where it is 4
ABI_CAND_SYM = (0, 1, 4, 2, 4, 1)


@functools.lru_cache(maxsize=None)
def abi_inputs():
    """2 objects, 2 views, P = 129 (a second pass of 2 rows), 6 meshes of which 3 are used, S = 5 DISTINCT symmetries per mesh
    (rotations about z by 72 degrees: one that n_sym excludes is seen if it is used), candidates = truth . inverse of symmetry
    ABI_CAND_SYM . noise."""
    from cosypose_amd import synthetic as syn
    rs = np.random.RandomState(SEED)
    scene = syn.make_ba_scene(SEED, 2, 2, ABI_P, p_visible=1.0)
    pts = rs.uniform(-1, 1, (ABI_N_MESH, ABI_P, 3)) * rs.uniform(0.03, 0.12, (ABI_N_MESH, 1, 3))
    sym = np.tile(np.eye(4), (ABI_N_MESH, ABI_S, 1, 1))
    for k in range(ABI_S):
        a = 2 * np.pi * k / ABI_S
        sym[:, k, :3, :3] = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    TWC = scene['cam_TWC']
    TWO = TWC[0] @ scene['cand_poses'][:2]                  # the first two candidates are objects 0, 1 in view 0
    TCW = np.linalg.inv(TWC)
    cand = np.stack([TCW[v] @ TWO[o] @ sym[m, (ABI_S - k) % ABI_S] @ syn._rigid_noise(rs, 0.03, 0.004)
                     for o, v, m, k in zip(ABI_CANDS['obj'], ABI_CANDS['view'], ABI_CANDS['mesh'], ABI_CAND_SYM)])
    TWO_9d = ba_ref.pose9d_of(TWO) + 3e-3 * rs.randn(2, 9)
    TCW_9d = ba_ref.pose9d_of(TCW) + 3e-3 * rs.randn(2, 9)
    return dict(TWO_9d=TWO_9d, TCW_9d=TCW_9d, cand_TCO=cand, K=scene['cam_K'], pts=pts, sym=sym)


FILL = 7.0               # sentinel of every output buffer


def run_abi(inp, ids, n_sym, device_ids=None):
    """cosy_ba_upload_ids / cosy_ba_align / cosy_ba_linearize on sentinel-filled outputs.  ids: dict obj, view, mesh (n_cand each,
    valid: the upload checks them) and obj_mesh; device_ids: {position in the device's id tensor: value} written past that check."""
    from cosypose_amd._lib import lib, check, ptr, stream
    l = lib()
    host = [np.ascontiguousarray(ids[k], dtype=np.int32) for k in ('obj', 'view', 'mesh', 'obj_mesh')]
    nc, no, nv = len(host[0]), len(inp['TWO_9d']), len(inp['TCW_9d'])
    n_mesh, P, S, n = inp['pts'].shape[0], inp['pts'].shape[1], inp['sym'].shape[1], 9 * (no + nv)
    d_ids = torch.zeros(3 * nc + no, dtype=torch.int32, device='cuda')
    check(l.cosy_ba_upload_ids(*(a.ctypes.data for a in host), nc, no, nv, n_mesh, ptr(d_ids), stream()))
    torch.cuda.synchronize()
    for pos, value in (device_ids or {}).items():
        d_ids[pos] = value
    t = {k: dev(inp[k]) for k in ('TWO_9d', 'TCW_9d', 'cand_TCO', 'K', 'pts', 'sym')}
    d_nsym = dev(np.asarray(n_sym, dtype=np.int32))

    def full(*shape):
        return torch.full(shape, FILL, dtype=torch.float64, device='cuda')
    out = dict(dists=full(nc), aligned=full(nc, 4, 4), errors=full(nc * 2 * P), loss=full(1), A=full(n, n), b=full(n),
               J_TWO=full(nc * 2 * P, 9), J_TCW=full(nc * 2 * P, 9), best=torch.full((nc,), 7, dtype=torch.int32, device='cuda'))
    ws_bytes = l.cosy_ba_workspace_bytes(nc, P, no, nv)
    assert ws_bytes >= 8 * max(n * n, nc * 190)
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device='cuda')
    check(l.cosy_ba_align(ptr(t['TWO_9d']), ptr(t['TCW_9d']), ptr(t['cand_TCO']), ptr(t['K']), ptr(d_ids), ptr(t['pts']), ptr(t['sym']),
                          ptr(d_nsym), nc, no, nv, n_mesh, P, S, ptr(out['dists']), ptr(out['best']), ptr(out['aligned']), stream()))
    check(l.cosy_ba_linearize(ptr(t['TWO_9d']), ptr(t['TCW_9d']), ptr(out['aligned']), ptr(t['K']), ptr(d_ids), ptr(t['pts']), nc, no, nv,
                              n_mesh, P, float(THRESHOLD), ptr(out['errors']), ptr(out['loss']), ptr(out['A']), ptr(out['b']),
                              ptr(out['J_TWO']), ptr(out['J_TCW']), ptr(ws), stream()))
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    out['loss'] = out['loss'][0]
    return out


def abi_reference(inp, ids, n_sym):
    return ba_ref.reference(inp['TWO_9d'], inp['TCW_9d'], inp['cand_TCO'], inp['K'], ids['obj'], ids['view'], ids['mesh'], ids['obj_mesh'],
                            inp['pts'], inp['sym'], n_sym, THRESHOLD)


@pytest.mark.parametrize('table', sorted(N_SYM_TABLES))
def test_c_abi_id_tables(table):
    """Three candidates on one (object, view) pair, summed by accumulate in candidate order; a candidate whose mesh (1, n_sym 3) is not
    its object's (0, n_sym 2): align must take the candidate's mesh, linearise the object's points; n_mesh = 6 with 3 meshes used;
    S = 5 above every n_sym ('below') and an n_sym = 7 clamped to S ('clamped').  Everything against ba_ref, as in (a).
    Measured on an MI355X: both tables dists 1.7e-16, errors 2.4e-15, loss <= 1.1e-15, J 4.1e-16, A 2.1e-15, b 1.2e-15 against
    (N + 64) eps = 2.4e-13; the clamp is seen (candidate 4 takes symmetry 4 only where n_sym = 7 is clamped to 5)."""
    inp, n_sym = abi_inputs(), N_SYM_TABLES[table]
    ids = dict(ABI_CANDS, obj_mesh=ABI_OBJ_MESH)
    ref = abi_reference(inp, ids, n_sym)
    assert ref['terms'] == 2 * ABI_P * 4                     # object 0's diagonal block sums four candidates
    assert (ref['best'] < np.minimum(np.asarray(n_sym)[list(ids['mesh'])], ABI_S)).all()
    assert ref['best'].tolist()[:4] == [0, 1, ref['best'][2], 2] and ref['best'][2] < 2 and (ref['best'][4] == 4) == (table == 'clamped')
    got = run_abi(inp, ids, n_sym)
    assert_linearisation(f'C ABI id tables, n_sym {table}', got, ref)
    assert same_bits(got, run_abi(inp, ids, n_sym))
    # had align taken the object's mesh for candidate 3, or linearise the candidate's, the reference would differ: both are visible
    swapped = abi_reference(inp, dict(ids, mesh=ABI_CANDS['mesh'][:3] + (0,) + ABI_CANDS['mesh'][4:]), n_sym)
    assert rel_err(swapped['dists'][3, swapped['best'][3]], ref['dists'][3, ref['best'][3]]) > 1e-3
    moved = abi_reference(inp, dict(ids, obj_mesh=(1, 2)), n_sym)
    assert rel_err(moved['errors'], ref['errors']) > 1e-3


def test_c_abi_mesh_without_symmetry():
    """A candidate whose mesh has n_sym = 0: its distance NaN, index -1, aligned pose NaN, its errors NaN and so the loss NaN (as
    torch.min(residuals, threshold) of the reference gives it); b is NaN in its object's and its view's rows only; the Jacobian does
    not depend on the candidate's pose, so A and every other candidate's outputs have the bits of a run in which that candidate has
    a symmetric mesh.  (Before this test the kernel's clamp `e2 < threshold ? e2 : threshold` turned a NaN residual into the
    threshold and the loss stayed finite; it is now `e2 > threshold ? threshold : e2`, the same value for every number.)"""
    inp, n_sym = abi_inputs(), N_SYM_TABLES['below']
    ids = dict(ABI_CANDS, obj_mesh=ABI_OBJ_MESH)
    base = run_abi(inp, ids, n_sym)
    got = run_abi(inp, dict(ids, mesh=ABI_CANDS['mesh'][:3] + (4,) + ABI_CANDS['mesh'][4:]), n_sym)
    rows = slice(3 * 2 * ABI_P, 4 * 2 * ABI_P)
    print('FIGURE mesh without symmetry: loss', got['loss'], 'dist', got['dists'][3], 'best', got['best'][3])
    assert np.isnan(got['dists'][3]) and got['best'][3] == -1 and np.isnan(got['aligned'][3]).all() and np.isnan(got['errors'][rows]).all()
    assert np.isnan(got['loss'])
    others = np.arange(6) != 3
    row_mask = np.repeat(others, 2 * ABI_P)
    for k in ('dists', 'best', 'aligned'):
        assert np.array_equal(got[k][others], base[k][others]), k
    for k in ('errors', 'J_TWO', 'J_TCW'):
        assert np.array_equal(got[k][row_mask], base[k][row_mask]), k
    assert np.array_equal(got['J_TWO'], base['J_TWO']) and np.array_equal(got['J_TCW'], base['J_TCW']) and np.array_equal(got['A'], base['A'])
    touched = np.zeros(36, dtype=bool)
    touched[0:9] = touched[27:36] = True                     # object 0, view 1 (objects first)
    assert np.isnan(got['b'][touched]).all() and np.array_equal(got['b'][~touched], base['b'][~touched])


BAD_IDS = [('obj', 2), ('obj', -1), ('view', 2), ('view', -5), ('mesh', ABI_N_MESH), ('mesh', 2 ** 30)]


def test_c_abi_skipped_candidate():
    """One candidate whose ids lie outside their tables, written into the device's id tensor past cosy_ba_upload_ids' check.  cand_ids
    in kernels_ba.hip tests o, v and the candidate's mesh against their tables BEFORE the only dependent read (obj_mesh[o]); align
    then returns and linearise writes the candidate's zero block and zero loss part, both inside their n_cand-sized buffers;
    accumulate only compares ids.  Its rows of dists / best / aligned / errors / J keep the sentinel fill, it adds exact zeros to A
    and b (the bits of a run without it), every other candidate's outputs have the bits of that run, and the loss is ba_ref's sum
    over the valid candidates divided by n_cand 2P (measured on an MI355X: 9.9e-16 for each of the six ids tried)."""
    inp, n_sym = abi_inputs(), N_SYM_TABLES['clamped']
    valid = dict(ABI_CANDS, obj_mesh=ABI_OBJ_MESH)
    without = run_abi(inp, valid, n_sym)
    ref = abi_reference(inp, valid, n_sym)
    assert_linearisation('skipped candidate: the run without it', without, ref)
    at, nc = 2, 7                                              # the bad candidate sits between two of (object 0, view 0)
    keep = np.arange(nc) != at
    ids = {k: valid[k][:at] + (0,) + valid[k][at:] for k in ('obj', 'view', 'mesh')}
    ids['obj_mesh'] = ABI_OBJ_MESH
    with_inp = dict(inp, cand_TCO=np.insert(inp['cand_TCO'], at, inp['cand_TCO'][0], axis=0))
    row_keep = np.repeat(keep, 2 * ABI_P)
    for n_case, (column, value) in enumerate(BAD_IDS):
        got = run_abi(with_inp, ids, n_sym, device_ids={('obj', 'view', 'mesh').index(column) * nc + at: value})
        loss_fig = rel_err(got['loss'], ref['loss'] * 6 / 7)
        print(f'FIGURE skipped candidate {column}={value}: loss {loss_fig:.2e}')
        assert got['dists'][at] == FILL and got['best'][at] == 7 and (got['aligned'][at] == FILL).all()
        for k in ('errors', 'J_TWO', 'J_TCW'):
            assert (got[k][~row_keep] == FILL).all(), (column, value, k)
            assert np.array_equal(got[k][row_keep], without[k]), (column, value, k)
        for k in ('dists', 'best', 'aligned'):
            assert np.array_equal(got[k][keep], without[k]), (column, value, k)
        assert np.array_equal(got['A'], without['A']) and np.array_equal(got['b'], without['b']), (column, value)
        assert loss_fig < min(LIN_TOL, LIN_CEILING)


# ---- d. the Cholesky solve across its thread tilings ---------------------------------------------------------------------------------
SOLVE_N = [1, 9, 18, 31, 32, 33, 1023, 1024, 1025, 1152]


@functools.lru_cache(maxsize=None)
def spd_system(n):
    """A = G^T G, G (2n x n) normal with columns scaled by logspace(0, -3, n); b normal"""
    rs = np.random.RandomState(1000 + n)
    G = torch.from_numpy(rs.randn(2 * n, n) * np.logspace(0, -3, n)[None])
    A = G.t() @ G
    return ((A + A.t()) / 2).contiguous(), torch.from_numpy(rs.randn(n))


def run_solve(A, b, lambd):
    from cosypose_amd._lib import lib, ptr, stream
    l = lib()
    n = len(b)
    blocks = max(2, -(-n // 9))
    ws_bytes = l.cosy_ba_workspace_bytes(1, 1, 1, blocks - 1)
    assert ws_bytes >= 8 * n * n
    dA, db = A.cuda(), b.cuda()
    h = torch.full((n + 64,), FILL, dtype=torch.float64, device='cuda')
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device='cuda')
    rc = l.cosy_ba_solve(ptr(dA), ptr(db), n, float(lambd), ptr(h), ptr(ws), stream())
    torch.cuda.synchronize()
    assert torch.equal(dA.cpu(), A) and torch.equal(db.cpu(), b)           # inputs untouched
    assert (h[n:] == FILL).all()                                           # nothing written past h
    return rc, h[:n].cpu()


@pytest.mark.parametrize('lambd', [1e-7, 1e-3, 1e7])
@pytest.mark.parametrize('n', SOLVE_N)
def test_solve_across_thread_tilings(n, lambd):
    """cosy_ba_solve on seeded positive definite systems at n = 1, 9, 18 (a trailing update with next to nothing to do), 31 / 32 / 33
    (around one 32 x 32 tile), 1023 / 1024 / 1025 (around the first trip of the 1024-thread loops) and 1152 (the documented limit):
    the rule of test_solve_residual_vs_torch_solve.  Measured on an MI355X, ratio ours / torch.linalg.solve: 0.37 ... 2.43 over the 30 cases
    (n >= 1023: 1.09 ... 1.69; at n = 1152 1.69 / 1.28 / 1.14 for lambda 1e-7 / 1e-3 / 1e7); residuals 0 ... 3.0e-13; at n = 1
    torch's residual is 0 and ours 1.8e-16, under the 10 n 2.2e-16 term."""
    A, b = spd_system(n)
    rc, h = run_solve(A, b, lambd)
    ours, theirs, bound = solve_rule(A, b, lambd, h)
    print(f'FIGURE solve tilings n={n} lambda={lambd:g}: residual {ours:.3e}, torch.linalg.solve {theirs:.3e}, '
          f'ratio {ours / max(theirs, 1e-300):.2f}, bound {bound:.3e}')
    assert rc == 0 and torch.isfinite(h).all()
    assert ours <= bound


def test_solve_indefinite_matrix_gives_non_finite_step():
    """A - 2 lambda_max I at n = 33: the entry reports success, h is non-finite (the first pivot is negative; the caller's loss test
    rejects such a step), A, b and the memory past h are untouched."""
    A, b = spd_system(33)
    M = (A - 2 * float(torch.linalg.eigvalsh(A)[-1]) * torch.eye(33, dtype=torch.float64)).contiguous()
    rc, h = run_solve(M, b, 1e-3)
    print('FIGURE indefinite solve: finite entries of h', int(torch.isfinite(h).sum()), 'of 33')
    assert rc == 0 and not torch.isfinite(h).all()


# ---- e. the float32 reprojected symmetric distance -----------------------------------------------------------------------------------
SDR_S = 4
SDR_N_SYM = (1, 4, 2, 3, 4, 1, 2, 3)


def sdr_inputs(P):
    from cosypose_amd import synthetic as syn
    rs = np.random.RandomState(SEED + P)
    n_obj = len(SDR_N_SYM)
    pts = (rs.uniform(-1, 1, (n_obj, P, 3)) * rs.uniform(0.03, 0.12, (n_obj, 1, 3))).astype(np.float32)
    sym = np.tile(np.eye(4), (n_obj, SDR_S, 1, 1))
    for k in range(SDR_S):                                  # S distinct symmetries for every object: no ties when all S count
        a = 2 * np.pi * k / SDR_S
        sym[:, k, :3, :3] = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    B = 24
    obj = np.concatenate((rs.permutation(n_obj), rs.randint(0, n_obj, B - n_obj)))
    T2 = syn.make_TCO(SEED + P, B).astype(np.float64)
    T1 = np.stack([T2[i] @ sym[obj[i], rs.randint(SDR_S)] @ syn._rigid_noise(rs, 0.03, 0.004) for i in range(B)])
    K = np.tile(np.array([[600., 0, 320], [0, 600., 240], [0, 0, 1]]), (B, 1, 1))
    return dict(T1=T1.astype(np.float32), T2=T2.astype(np.float32), K=K.astype(np.float32), obj=obj, pts=pts, sym=sym.astype(np.float32))


def run_sdr(inp, B, obj, n_sym):
    from cosypose_amd._lib import lib, check, ptr, stream
    n_obj, P = inp['pts'].shape[:2]
    t = {k: dev(inp[k][:B] if k in ('T1', 'T2', 'K') else inp[k]) for k in ('T1', 'T2', 'K', 'pts', 'sym')}
    d_obj = None if obj is None else dev(np.asarray(obj, dtype=np.int32))
    d_nsym = None if n_sym is None else dev(np.asarray(n_sym, dtype=np.int32))
    d = torch.full((B,), FILL, device='cuda')
    best = torch.full((B,), 7, dtype=torch.int32, device='cuda')
    S12 = torch.full((B, 4, 4), FILL, device='cuda')
    check(lib().cosy_symmetric_distance_reprojected(ptr(t['T1']), ptr(t['T2']), ptr(t['K']), ptr(d_obj), ptr(t['pts']), ptr(t['sym']),
                                                    ptr(d_nsym), B, n_obj, P, SDR_S, ptr(d), ptr(best), ptr(S12), stream()))
    torch.cuda.synchronize()
    return d.cpu().numpy(), best.cpu().numpy(), S12.cpu().numpy()


@pytest.mark.parametrize('P', [1, 63, 255, 256, 257, 1000])
def test_reprojected_distance_float32(P):
    """cosy_symmetric_distance_reprojected (float32) against ba_ref's float64 evaluation of the same formula on the widened inputs:
    P = 1 and 63 (whole waves pass the neutral element to the workgroup sum), 255 / 256 / 257 (around the 256-point stride), 1000;
    objects with n_sym = 1, = S and in between, the n_sym table absent (all S count), obj_id absent (item b reads row b), a
    permutation and repeats.  Distances within DIST_TOL (max-norm, as in test_bundle_adjustment.py), the index exact on every item
    whose margin to the runner-up exceeds 2 DIST_TOL x the runner-up (each distance may move by DIST_TOL of itself), S12 the chosen
    table row exactly.  The inputs are chosen so that the reference alone shows no thin margin.  Measured on an MI355X: worst distance
    figure with the n_sym table 1.1e-6 (P = 1), without it 6.1e-6 (P = 1: one point, no averaging of the pixel rounding; 3.2e-6 ...
    5.3e-6 at the other P); no thin margin anywhere (smallest 0.23 px relative to a runner-up of 4.4 px), every index and S12 exact."""
    inp = sdr_inputs(P)
    n_obj = len(SDR_N_SYM)
    cases = dict(permutation_and_repeats=(24, inp['obj'], SDR_N_SYM), no_obj_id=(n_obj, None, SDR_N_SYM), no_n_sym=(24, inp['obj'], None))
    for name, (B, obj, n_sym) in cases.items():
        dists, best, margin, S12 = ba_ref.reprojected_distance_float32(inp['T1'][:B], inp['T2'][:B], inp['K'][:B], obj, inp['pts'],
                                                                       inp['sym'], n_sym)
        want = dists[np.arange(B), best]
        runner_up = want + margin                             # inf where one symmetry counts
        thin = ~(margin > 2 * DIST_TOL * np.where(np.isfinite(runner_up), runner_up, 0.))
        got_d, got_best, got_S12 = run_sdr(inp, B, obj, n_sym)
        fig = rel_err(got_d, want)
        print(f'FIGURE reprojected float32 P={P} {name}: dists {fig:.2e}, thin margins {int(thin.sum())} of {B}, '
              f'smallest margin {float(margin.min()):.3g} px, chosen {sorted(set(best.tolist()))}')
        assert thin.mean() == 0.                              # shown by the reference alone; the kernel may leave out at most 5 %
        assert np.array_equal(got_best[~thin], best[~thin]) and thin.mean() <= 0.05
        assert np.array_equal(got_S12[~thin], S12[~thin])
        assert got_d.dtype == np.float32 and fig < DIST_TOL
        if n_sym is None:
            assert len(set(best.tolist())) > 2
