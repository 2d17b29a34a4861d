"""The host side of the batched bundle adjustment (cosypose_amd/bundle_adjustment.py: _batch_plan, solve_problems' refusals) on
CPU-tensor problems: no device is needed, and none is touched."""
import numpy as np
import pytest

import ba_batch_case as bc

SUBSETS = [((0, 1, 2, 3, 4), (0, 1, 2, 3, 4, 5)), ((2,), (1,)), ((0, 3), (0, 2, 4)), ((1, 2, 4), (5, 3, 1, 0))]


@pytest.fixture(scope='module')
def problems():
    from cosypose_amd import synthetic as syn
    scene = syn.make_ba_scene(11, 6, 5, 31, p_visible=1.0)
    mesh_db = bc.mesh_db_of(scene)
    return [bc.problem_on(bc.sub_scene(scene, v, o), mesh_db) for v, o in SUBSETS]


@pytest.fixture
def no_device(monkeypatch):
    """any call into the library or any device check fails the test"""
    from cosypose_amd import bundle_adjustment as ba

    def boom(*a, **k):
        raise AssertionError('the device side was reached')
    monkeypatch.setattr(ba, 'lib', boom)
    monkeypatch.setattr(ba, 'require_device', boom)


def test_batch_plan_tables(problems):
    from cosypose_amd.bundle_adjustment import _batch_plan
    plan = _batch_plan(problems)
    G = len(problems)
    assert plan['G'] == G and [len(plan[k]) for k in ('cand_off', 'obj_off', 'view_off', 'par_off', 'A_off')] == [G + 1] * 5
    sizes = dict(cand_off=[p.n_candidates for p in problems], obj_off=[p.n_objects for p in problems], view_off=[p.n_views for p in problems],
                 par_off=[9 * (p.n_objects + p.n_views) for p in problems], A_off=[(9 * (p.n_objects + p.n_views)) ** 2 for p in problems])
    for k, s in sizes.items():          # exclusive prefix sums
        assert plan[k][0] == 0 and np.array_equal(np.diff(plan[k]), s), k
    assert [p.n_candidates for p in problems] == [30, 1, 6, 12]          # the subsets are what they say (every object visible everywhere)
    assert plan['n'].tolist() == sizes['par_off'] and plan['max_blocks'] == 11
    assert plan['A_off'][-1] == sum(n * n for n in sizes['par_off']) and plan['A_off'].dtype == np.int64
    assert all(plan[k].dtype == np.int32 and plan[k].flags.c_contiguous for k in ('cand_obj', 'cand_view', 'cand_mesh', 'obj_mesh', 'cand_off',
                                                                                  'obj_off', 'view_off'))
    assert len(plan['cand_obj']) == len(plan['cand_view']) == len(plan['cand_mesh']) == plan['cand_off'][-1]
    assert len(plan['obj_mesh']) == plan['obj_off'][-1]
    for g, p in enumerate(problems):    # every table = the problem's own id map shifted by its offsets
        c0, c1, o0, o1 = plan['cand_off'][g], plan['cand_off'][g + 1], plan['obj_off'][g], plan['obj_off'][g + 1]
        assert np.array_equal(plan['cand_obj'][c0:c1] - o0, p.cand_obj_ids)
        assert np.array_equal(plan['cand_view'][c0:c1] - plan['view_off'][g], p.cand_view_ids)
        assert np.array_equal(plan['cand_mesh'][c0:c1], [p.mesh_db.label_to_id[l] for l in p.cand_labels])
        assert np.array_equal(plan['obj_mesh'][o0:o1], [p.mesh_db.label_to_id[l] for l in p.obj_infos['label']])
        assert plan['cand_obj'][c0:c1].min() >= o0 and plan['cand_obj'][c0:c1].max() < o1


def test_batch_plan_is_order_dependent_only_through_offsets(problems):
    from cosypose_amd.bundle_adjustment import _batch_plan
    fwd, rev = _batch_plan(problems), _batch_plan(problems[::-1])
    G = len(problems)
    for g in range(G):
        r = G - 1 - g
        a = fwd['cand_obj'][fwd['cand_off'][g]:fwd['cand_off'][g + 1]] - fwd['obj_off'][g]
        b = rev['cand_obj'][rev['cand_off'][r]:rev['cand_off'][r + 1]] - rev['obj_off'][r]
        assert np.array_equal(a, b)


def test_refusals_touch_no_device(problems, no_device):
    from cosypose_amd import synthetic as syn
    from cosypose_amd.bundle_adjustment import solve_problems, _batch_plan
    assert solve_problems([]) == []
    other = syn.make_ba_scene(12, 3, 2, 31)
    stranger = bc.problem_on(other, bc.mesh_db_of(other))
    with pytest.raises(ValueError, match='mesh_db'):
        solve_problems([problems[0], stranger])
    with pytest.raises(ValueError, match='mesh_db'):
        _batch_plan([stranger, problems[1]])
    big_scene = syn.make_ba_scene(3, 122, 8, 8, p_visible=0.2)            # 130 blocks > 128
    mesh_db = bc.mesh_db_of(big_scene)
    big, small = bc.problem_on(big_scene, mesh_db), bc.problem_on(bc.sub_scene(big_scene, (0, 1), (0, 1, 2)), mesh_db)
    with pytest.raises(ValueError, match='> 128'):
        solve_problems([small, big])
    with pytest.raises(ValueError):
        solve_problems(problems, n_iterations=0)
    with pytest.raises(ValueError):
        solve_problems(problems, poll_every=0)


def test_cpu_problems_are_refused_not_emulated(problems):
    """a valid batch of CPU tensors: there is no CPU fallback"""
    from cosypose_amd._lib import CosyHipError
    from cosypose_amd.bundle_adjustment import solve_problems
    with pytest.raises(CosyHipError, match='ROCm device only'):
        solve_problems(problems)


def test_c_side_refuses_bad_tables_before_any_copy():
    """cosy_ba_batch_upload checks the host tables first: return codes only, nothing is copied (the device pointer is never used)"""
    import ctypes
    from cosypose_amd._lib import lib
    l = lib()
    EINVAL, ESIZE = -1, -4
    arr = lambda *v: (ctypes.c_int * len(v))(*v)
    a_total, max_blocks = ctypes.c_longlong(0), ctypes.c_int(0)
    fake = ctypes.c_void_p(256)       # never dereferenced: every call below is refused

    def upload(cand_obj=arr(0, 1, 2), cand_view=arr(0, 0, 1), cand_mesh=arr(0, 1, 1), obj_mesh=arr(0, 1, 1), cand_off=arr(0, 2, 3),
               obj_off=arr(0, 2, 3), view_off=arr(0, 1, 2), G=2, n_mesh=2, table=fake):
        a = lambda x: ctypes.addressof(x) if x is not None else None
        return l.cosy_ba_batch_upload(a(cand_obj), a(cand_view), a(cand_mesh), a(obj_mesh), a(cand_off), a(obj_off), a(view_off), G, n_mesh,
                                      table, ctypes.byref(a_total), ctypes.byref(max_blocks), None)
    assert upload(cand_obj=arr(0, 2, 2)) == EINVAL and b'problem 0, candidate 1: object row 2' in l.cosy_last_error()   # another problem's row
    assert upload(cand_obj=arr(0, 1, 1)) == EINVAL and b'problem 1, candidate 2: object row 1' in l.cosy_last_error()
    assert upload(cand_view=arr(0, 1, 1)) == EINVAL and b'view row 1' in l.cosy_last_error()
    assert upload(cand_view=arr(0, 0, -1)) == EINVAL
    assert upload(cand_mesh=arr(0, 2, 1)) == EINVAL and b'mesh id 2' in l.cosy_last_error()
    assert upload(obj_mesh=arr(0, 1, -1)) == EINVAL and b'object 2' in l.cosy_last_error()
    assert upload(cand_off=arr(0, 3, 3)) == EINVAL and b'problem 1: 0 candidates' in l.cosy_last_error()
    assert upload(obj_off=arr(1, 2, 3)) == EINVAL and upload(view_off=arr(0, 2, 2)) == EINVAL
    assert upload(G=0) == EINVAL and upload(n_mesh=0) == EINVAL and upload(table=None) == EINVAL and upload(cand_obj=None) == EINVAL
    assert upload(obj_off=arr(0, 2, 130), view_off=arr(0, 1, 3)) == ESIZE and b'problem 1' in l.cosy_last_error() and b'> 128' in l.cosy_last_error()
    assert l.cosy_ba_batch_table_bytes(0, 3, 3) == 0 and l.cosy_ba_batch_table_bytes(2, 3, 3) >= 4 * (4 * 3 + 3 + 9) + 8 * 3
    assert l.cosy_ba_batch_workspace_bytes(3, 5, 2 * 18 * 18 + 27 * 27) >= 8 * (3 * (189 + 1 + 16) + 2 * (2 * 18 * 18 + 27 * 27) + 45)
    assert l.cosy_ba_batch_workspace_bytes(0, 5, 100) == 0
    for fn, args in ((l.cosy_ba_batch_linearize, (None, 0, None)), (l.cosy_ba_batch_solve_step, (None, None)),
                     (l.cosy_ba_batch_iterate, (None, 0, 1, None))):
        assert fn(*args) == EINVAL and b'null batch' in l.cosy_last_error()
    assert l.cosy_ba_batch_decide(None, 1, 9., 11., 1e-5, None, 0, 0, None, None, None, None, None) == EINVAL
    assert l.cosy_ba_batch_decide(fake, 1, 0., 11., 1e-5, None, 0, 0, None, None, None, None, None) == EINVAL
    assert l.cosy_ba_batch_decide(fake, 1, 9., 11., 1e-5, None, 0, 0, fake, None, None, None, None) == EINVAL       # states without the table
    assert l.cosy_ba_batch_record(None, 1, 0, 4, None, 0, 0, 0, None, None, fake, fake, fake, None, None, None) == EINVAL
    assert l.cosy_ba_batch_record(fake, 1, 0, 4, None, 0, 0, 0, None, None, fake, fake, fake, fake, None, None) == EINVAL
    assert l.cosy_ba_batch_record(fake, 1, 0, 0, None, 0, 0, 0, None, None, fake, fake, fake, None, None, None) == EINVAL
