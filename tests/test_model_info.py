"""Object models on the GPU (cosypose_amd/model_info.py, csrc/kernels_models.hip) against the numpy float64 restatement of
tests/models_ref.py, which tests/test_model_info_host.py pins to SciPy's cdist bit for bit.  The contract is DESIGN.md section 20.

Every comparison is EQUALITY: the diameter's float64 bits, the vertex pair, the box.  T is the kernel's tile edge; the sizes sit on
both sides of one tile and of several, so that models with one diagonal tile, with partial last tiles and with off-diagonal tiles all
pass through one grid together.
"""
import numpy as np
import pytest
import torch

import models_ref as mr

pytestmark = pytest.mark.gpu

KEYS = ('diameter', 'min_x', 'min_y', 'min_z', 'size_x', 'size_y', 'size_z', 'diameter_ids')


def T():
    from cosypose_amd.model_info import TILE
    return TILE


def mix_sizes():
    t = T()
    return [1, 2, t - 1, t, t + 1, 2 * t + 3, 3 * t + 1]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def assert_equal_infos(got, models):
    assert len(got) == len(models)
    for k, (g, p) in enumerate(zip(got, models)):
        want = mr.info_ref(p)
        print(k, len(p), g['diameter'], g['diameter_ids'], want['diameter'], want['diameter_ids'])
        assert tuple(g) == KEYS and all(type(g[key]) is float for key in KEYS[:7]) and all(type(x) is int for x in g['diameter_ids'])
        for key in KEYS:
            assert g[key] == want[key], (k, key, g[key], want[key])


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['float32', 'float64'])
def test_ragged_mix_equals_the_restatement(dtype):
    from cosypose_amd import model_info
    models = mr.make_models(5, mix_sizes(), scale=100.0, dtype=dtype)
    if dtype == np.float64:
        assert all((p != p.astype(np.float32)).all() for p in models)                 # coordinates that no float32 holds
    got = model_info([dev(p) for p in models])
    assert_equal_infos(got, models)
    assert got[0]['diameter'] == 0.0 and got[0]['diameter_ids'] == (0, 0) and got[1]['diameter_ids'] == (0, 1)
    # NumPy arrays are uploaded; a model's row does not depend on what else is in the call
    alone = model_info([models[5]])
    assert alone[0] == got[5]
    assert np.array_equal(model_info.diameters([dev(p) for p in models[:4]]), np.array([g['diameter'] for g in got[:4]]))


def test_empty_list():
    from cosypose_amd import model_info
    assert model_info([]) == [] and model_info.diameters([]).shape == (0,)


def tie_models():
    """-> (models, expected pairs).  A cloud of radius < 2 around the origin and far vertices at (+-50, 0, 0): every (+, -) pair is a
    diameter, exactly 100 apart"""
    t = T()
    rs = np.random.RandomState(9)
    A, B = np.array([50, 0, 0], np.float32), np.array([-50, 0, 0], np.float32)

    def cloud(V, plus, minus):
        p = rs.uniform(-1, 1, (V, 3)).astype(np.float32)
        p[plus], p[minus] = A, B
        return p
    c = mr.cube()
    models = [c, np.concatenate([c, c[7:8]]), np.concatenate([c[7:8], c]),
              cloud(2 * t + 3, [2 * t + 1], [2 * t + 2]),                       # the pair in the last, partial tile
              cloud(3 * t + 1, [t + 5], [t + 100]),                             # inside one diagonal tile
              cloud(3 * t + 1, [3, t + 5], [t + 7, 2 * t + 1]),                 # four equal pairs in four tiles, one of them diagonal
              cloud(2 * t, [t - 1, 2 * t - 1], [0, t]),                         # i > j within the equal pairs: (0, t - 1) is the smallest
              np.zeros((t + 2, 3), np.float32)]                                 # every pair attains 0
    pairs = [(0, 7), (0, 7), (0, 1), (2 * t + 1, 2 * t + 2), (t + 5, t + 100), (3, t + 7), (0, t - 1), (0, 1)]
    return models, pairs


def test_ties_give_the_lexicographically_smallest_pair():
    from cosypose_amd import model_info
    models, pairs = tie_models()
    got = model_info([dev(p) for p in models])
    for k, (g, p, want) in enumerate(zip(got, models, pairs)):
        print(k, len(p), g['diameter'], g['diameter_ids'], want)
        assert g['diameter_ids'] == want == mr.diameter_ref(p)[1], k
    assert [g['diameter'] for g in got] == [np.sqrt(12.0)] * 3 + [100.0] * 4 + [0.0]
    # the same models in another order and in another call: the same pairs
    again = model_info([dev(p) for p in models[::-1]])[::-1]
    assert again == got


def test_a_tile_list_longer_than_the_grid():
    """257 tile rows = 33 153 tiles, more than the 32 768 workgroups of the pair kernel (MI_MAX_GRID): the tiles past the grid are
    walked in a second round.  The answer is known by construction (no V x V reference): a cloud of radius < 2 and three far vertices,
    the diameter between vertex 5 and the LAST vertex, whose tile (row 0, column 256) has the list index 32 896; a vertex equal to
    vertex 5 further down gives a second, larger pair of the same length."""
    from cosypose_amd import model_info
    t = T()
    V = 256 * t + 1
    assert (V + t - 1) // t == 257 and 257 * 258 // 2 > 32768 and 256 * 257 // 2 + 0 >= 32768
    p = np.random.RandomState(1).uniform(-1, 1, (V, 3)).astype(np.float32)
    p[5] = p[70000] = [-50, 0, 0]
    p[V - 1] = [50, 0, 0]
    got = model_info([dev(p), dev(mr.cube())])
    print(got[0])
    assert got[0]['diameter'] == 100.0 and got[0]['diameter_ids'] == (5, V - 1) and got[1]['diameter_ids'] == (0, 7)
    assert [got[0]['min_x'], got[0]['size_x']] == [-50.0, 100.0] and got[0]['min_y'] == float(p[:, 1].min())


def test_32_random_models_hold_the_uncontracted_bits():
    """V = 1500, scale 100, float64 coordinates.  Checked on the CPU while writing this test: with the sum contracted into fused
    multiply-adds -- fma(dz, dz, fma(dy, dy, dx * dx)), what the compiler makes of it without -ffp-contract=off -- the largest squared
    distance differs from the restatement's on 3 of these 32 models (and with fma(dx, dx, dy * dy) + dz * dz on 2), so a build that
    drops the flag fails here.  With float32-valued coordinates it differs on NONE: there dx is short enough for dx * dx to be exact."""
    from cosypose_amd import model_info
    models = mr.make_models(11, [1500] * 32, scale=100.0, dtype=np.float64)
    got = model_info([dev(p) for p in models])
    ref = [mr.diameter_ref(p) for p in models]
    bad = [k for k in range(32) if got[k]['diameter'] != np.sqrt(ref[k][0]) or got[k]['diameter_ids'] != ref[k][1]]
    print('models that differ:', bad)
    assert not bad
    for g, p in zip(got, models):
        lo, size = mr.box_ref(p)
        assert [g['min_x'], g['min_y'], g['min_z']] == lo.tolist() and [g['size_x'], g['size_y'], g['size_z']] == size.tolist()


def test_a_nan_vertex_raises_and_names_the_model():
    from cosypose_amd import model_info
    models = mr.make_models(2, [40, T() + 9, 17, 5], scale=10.0)
    models[2][11, 1] = np.nan
    with pytest.raises(ValueError, match=r'model 2 has 1 non-finite coordinates$'):
        model_info([dev(p) for p in models])
    models[1][T() + 3] = [np.inf, 0, -np.inf]
    with pytest.raises(ValueError, match=r'model 1 has 2 non-finite coordinates \(and models \[2\] too\)'):
        model_info([dev(p) for p in models])
    assert_equal_infos(model_info([dev(models[0]), dev(models[3])]), [models[0], models[3]])


def test_two_identical_calls_give_identical_results():
    from cosypose_amd import model_info
    models, _ = tie_models()
    verts = [dev(p) for p in models + mr.make_models(4, [3 * T() + 1, 700], scale=1000.0)]
    a, b = model_info(verts), model_info(verts)
    assert a == b
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = model_info(verts)
    assert c == a


def test_end_to_end_mesh_database_feeds_the_meters():
    """vertices alone -> MeshDataBase.from_models_info(None, ...) -> batched().cuda() -> BopModels.from_mesh_db and PoseErrorMeter"""
    from cosypose_amd import MeshDataBase, BopModels, PoseErrorMeter
    box = np.array([[x, y, z] for x in (-40, 40) for y in (-30, 30) for z in (-20, 20)], np.float32)            # mm
    tet = np.array([[0, 0, 0], [90, 0, 0], [0, 60, 0], [0, 0, 30]], np.float32)
    box_f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]], np.int32)
    tet_f = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)
    db = MeshDataBase.from_models_info(None, {3: box, 8: dev(tet)})
    want = [float(np.sqrt(mr.diameter_ref(box)[0])), float(np.sqrt(mr.diameter_ref(tet)[0]))]
    assert want[0] == np.sqrt(80.0 ** 2 + 60.0 ** 2 + 40.0 ** 2) and want[1] == np.sqrt(90.0 ** 2 + 60.0 ** 2)
    assert [r['diameter'] for r in db.infos.values()] == want and [r['diameter_m'] for r in db.infos.values()] == [w * 0.001 for w in want]
    mesh_db = db.batched().cuda()
    assert list(mesh_db.labels) == ['obj_000003', 'obj_000008'] and mesh_db.points.shape == (2, 8, 3) and mesh_db.points.is_cuda
    assert mesh_db.infos['obj_000008']['n_points'] == 4 and mesh_db.infos['obj_000008']['n_sym'] == 1
    verts_m = [box * np.float32(0.001), tet * np.float32(0.001)]
    models = BopModels.from_mesh_db(mesh_db, verts_m, [box_f, tet_f])
    assert models.diameters.tolist() == [w * 0.001 for w in want]
    # the default fallback (the box diagonal) overstates the tetrahedron's diameter; the box's own is its diagonal
    fallback = BopModels(list(mesh_db.labels), verts_m, [box_f, tet_f]).diameters
    assert fallback[1] > models.diameters[1] * 1.03 and abs(fallback[0] - models.diameters[0]) < 1e-6
    meter = PoseErrorMeter(mesh_db, error_type='ADD')
    eye = torch.eye(4).repeat(2, 1, 1)
    moved = eye.clone()
    moved[:, 0, 3] = torch.tensor([0.01, 0.02])
    err = meter.compute_errors(moved, eye, ['obj_000003', 'obj_000008'])['norm_avg'].cpu().numpy()
    print(err, meter.mesh_db.infos['obj_000003']['diameter_m'])
    assert np.abs(err - np.array([0.01, 0.02])).max() < 1e-6
    assert meter.mesh_db.infos['obj_000003']['diameter_m'] == want[0] * 0.001
