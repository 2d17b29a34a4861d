"""CPU tests of the object models: the numpy restatement of the diameter (tests/models_ref.py) against SciPy's cdist bit for bit,
make_bop_symmetries against a closed form, MeshDataBase.batched() against the reference's bytes as its text defines them (shared
RandomState(0) padding, float64 scaling before the float32 rounding, identity-padded symmetries, box corners), the rows of
from_models_info, io_formats.models_info_rows, and the C ABI's host-side argument checks.  No GPU."""
import ctypes
import json
import pathlib
import re

import numpy as np
import pytest
import torch

import models_ref as mr

REPO = pathlib.Path(__file__).resolve().parent.parent


# ---- the restatement against SciPy (no package code) --------------------------------------------------------------------------------------
@pytest.mark.parametrize('scale', [0.1, 1.0, 100.0, 1000.0])
def test_restatement_equals_scipy_cdist_bit_for_bit(scale):
    cdist = pytest.importorskip('scipy.spatial.distance').cdist
    single_differs = 0
    for V in (1, 2, 63, 64, 65, 257, 1500, 4097):
        p = mr.make_models(V, [V], scale=scale)[0]                  # float32-valued coordinates
        s, (i, j) = mr.diameter_ref(p)
        p64 = p.astype(np.float64)
        want = cdist(p64, p64)
        assert np.sqrt(s) == want.max(), (V, scale, np.sqrt(s), want.max())
        assert (i, j) == tuple(int(x) for x in np.unravel_index(np.argmax(np.triu(want)), want.shape)) and (i < j or V == 1)
        if V >= 2:
            d32 = p[i] - p[j]                                        # the same pair in float32 arithmetic
            single_differs += np.sqrt(np.float64((d32[0] * d32[0] + d32[1] * d32[1]) + d32[2] * d32[2])) != want.max()
    print(scale, 'float32 arithmetic differs on', single_differs, 'of 7 models')
    assert single_differs > 0                                       # a single-precision kernel cannot pass


def test_restatement_ties_and_single_vertex():
    c = mr.cube()
    assert mr.diameter_ref(c) == (12.0, (0, 7))
    assert mr.diameter_ref(np.concatenate([c, c[7:8]])) == (12.0, (0, 7))          # a duplicate of corner 7 at index 8: (0, 7) < (0, 8)
    assert mr.diameter_ref(np.concatenate([c[7:8], c])) == (12.0, (0, 1))          # the duplicate first: (0, 1) < (1, 8)
    assert mr.diameter_ref(c[:1]) == (0.0, (0, 0))
    assert mr.diameter_ref(np.zeros((5, 3))) == (0.0, (0, 1))                       # all equal: every pair is a diameter
    lo, size = mr.box_ref(c + np.float32(3))
    assert lo.tolist() == [3, 3, 3] and size.tolist() == [2, 2, 2]


# ---- make_bop_symmetries ------------------------------------------------------------------------------------------------------------------
FLIP_Z = [-1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1, 30.0, 0, 0, 0, 1]          # rotation by pi about z, translation (0, 0, 30) in the model's units
FLIP_X = [1, 0, 0, 5.0, 0, -1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1]


def cont(axis_id):
    return dict(axis=np.eye(3, dtype=int)[axis_id].tolist(), offset=[0, 0, 0])


@pytest.mark.parametrize('discrete,axes,n,count', [([], [], 8, 1), ([FLIP_Z], [], 8, 2), ([FLIP_Z, FLIP_X], [], 64, 3), ([], [2], 1, 1), ([], [2], 8, 8),
                                                     ([], [0], 64, 64), ([], [1], 8, 8), ([FLIP_Z], [2], 8, 16), ([FLIP_Z, FLIP_X], [0, 2], 8, 48)])
def test_make_bop_symmetries_against_the_closed_form(discrete, axes, n, count):
    from cosypose_amd import make_bop_symmetries
    d = dict(symmetries_discrete=discrete, symmetries_continuous=[cont(a) for a in axes])
    keep = json.dumps(d)
    got = make_bop_symmetries(d, n_symmetries_continuous=n, scale=0.001)
    want = mr.symmetries_ref(discrete, axes, n, 0.001)
    err = np.abs(got - want).max()
    print(len(got), err)
    assert got.dtype == np.float64 and got.shape == (count, 4, 4) == want.shape and err <= 1e-12
    assert np.array_equal(got[0], np.eye(4)) and json.dumps(d) == keep                   # the identity first, the input untouched
    if discrete and not axes:
        assert got[1][2, 3] == 30.0 * 0.001 and np.array_equal(got[1][:3, :3], np.array(FLIP_Z, float).reshape(4, 4)[:3, :3])
    if discrete and axes:
        # the continuous symmetry is the inner loop: entries [0, n_c) belong to the identity, the next n_c to the first discrete symmetry
        n_c = n * len(axes)
        assert np.abs(got[n_c] - want[n_c]).max() <= 1e-12 and abs(got[n_c][2, 3] - 0.03) <= 1e-15 and abs(got[1][2, 3]) == 0.0


def test_make_bop_symmetries_missing_keys_and_assertions():
    from cosypose_amd import make_bop_symmetries
    assert np.array_equal(make_bop_symmetries({}), np.eye(4)[None])
    with pytest.raises(AssertionError):
        make_bop_symmetries(dict(symmetries_continuous=[dict(axis=[1, 1, 0], offset=[0, 0, 0])]))
    with pytest.raises(AssertionError):
        make_bop_symmetries(dict(symmetries_continuous=[dict(axis=[0, 0, 1], offset=[0, 0, 1.0])]))
    with pytest.raises(AssertionError):
        make_bop_symmetries(dict(symmetries_continuous=[dict(axis=[0.5, 0.5, 0], offset=[0, 0, 0])]))       # sums to 1, but no single 1


# ---- MeshDataBase --------------------------------------------------------------------------------------------------------------------------
def rows_and_verts():
    rs = np.random.RandomState(3)
    sizes = [7, 12, 12, 5, 9]
    verts = [(rs.standard_normal((V, 3)) * 80).astype(np.float32) for V in sizes]
    verts[4] = verts[4].astype(np.float64) * (1.0 + 2.0 ** -40)          # float64 vertices that no float32 holds
    rows = [dict(label=f'obj_{k + 1:06d}', mesh_units='mm', symmetries_discrete=[], symmetries_continuous=[], is_symmetric=False,
                 diameter=100.0 + k, diameter_m=(100.0 + k) * 0.001) for k in range(5)]
    rows[1].update(symmetries_discrete=[FLIP_Z], is_symmetric=True)
    rows[3].update(symmetries_continuous=[cont(2)], is_symmetric=True)
    rows[2]['mesh_units'] = 'm'
    return rows, verts, sizes


def test_batched_reproduces_the_reference_bytes():
    from cosypose_amd import MeshDataBase, BatchedMeshes
    rows, verts, sizes = rows_and_verts()
    db = MeshDataBase(rows, [torch.from_numpy(v) if k % 2 else v for k, v in enumerate(verts)])       # CPU tensors and arrays alike
    b = db.batched(n_sym=4)
    assert isinstance(b, BatchedMeshes) and b.points.dtype == torch.float32 and b.symmetries.dtype == torch.float32
    assert b.points.shape == (5, 12, 3) and b.symmetries.shape == (5, 4, 4, 4) and list(b.labels) == [r['label'] for r in rows]
    # ONE RandomState(0), consumed in object order and only by the objects that need padding (objects 1 and 2 are full)
    rng = np.random.RandomState(0)
    for k, (v, V) in enumerate(zip(verts, sizes)):
        scaled = v.astype(np.float64) * (1.0 if k == 2 else 0.001)
        want = scaled if V == 12 else np.concatenate([scaled, scaled[rng.choice(np.arange(V), size=12 - V)]])
        assert np.array_equal(b.points[k].numpy(), want.astype(np.float32)), k
    assert np.array_equal(b.points[0, :7].numpy(), (verts[0].astype(np.float64) * 0.001).astype(np.float32))
    # scaling in float64 and ONE rounding: not float32(v) * float32(0.001)
    assert not np.array_equal(b.points[0, :7].numpy(), verts[0] * np.float32(0.001))
    assert np.array_equal(b.points[4, :9].numpy(), (verts[4] * 0.001).astype(np.float32))
    n_sym = [1, 2, 1, 4, 1]
    for k, r in enumerate(rows):
        info = b.infos[r['label']]
        assert info['n_points'] == sizes[k] and info['n_sym'] == n_sym[k] and info['diameter_m'] == r['diameter_m']
        assert np.array_equal(b.symmetries[k, n_sym[k]:].numpy(), np.tile(np.eye(4, dtype=np.float32), (4 - n_sym[k], 1, 1)))
        want = mr.symmetries_ref(r['symmetries_discrete'], [2] if r['symmetries_continuous'] else [], 4, 1.0 if k == 2 else 0.001)
        assert np.abs(b.symmetries[k, :n_sym[k]].numpy() - want).max() <= 1e-7
    assert b.n_sym_mapping == {r['label']: n for r, n in zip(rows, n_sym)}
    assert 'n_points' not in db.infos['obj_000001'] and 'n_points' not in rows[0]          # the database's own rows are not touched
    assert b.select(['obj_000004', 'obj_000001']).points.shape == (2, 12, 3)


def test_batched_aabb_corners_and_refusals():
    from cosypose_amd import MeshDataBase
    rows, verts, sizes = rows_and_verts()
    db = MeshDataBase(rows, verts)
    a = db.batched(aabb=True, n_sym=4)
    assert a.points.shape == (5, 8, 3) and all(a.infos[r['label']]['n_points'] == 8 for r in rows)
    for k, v in enumerate(verts):
        want = (mr.aabb_ref(v.astype(np.float64)) * (1.0 if k == 2 else 0.001)).astype(np.float32)
        assert np.array_equal(a.points[k].numpy(), want), k
    # the corner order of BatchedMeshes.aabb() on the full table (object 1 has no padding: same vertices either way)
    assert np.array_equal(db.batched(n_sym=4).aabb().points[1].numpy(), a.points[1].numpy())
    with pytest.raises(NotImplementedError, match='sample_surface'):
        db.batched(resample_n_points=100)
    rows[0]['mesh_units'] = 'cm'
    with pytest.raises(ValueError, match='Unit not supported'):
        MeshDataBase(rows, verts).batched()


def test_from_models_info_builds_the_rows_of_bop_object_dataset():
    from cosypose_amd import MeshDataBase
    _, verts, _ = rows_and_verts()
    info = {'1': dict(diameter=172.063, min_x=-1.0, size_x=2.0), '5': dict(diameter=50.5, symmetries_discrete=[FLIP_Z]),
            '12': dict(diameter=80.25, symmetries_continuous=[cont(2)])}
    db = MeshDataBase.from_models_info(info, {1: verts[0], 12: verts[2], 5: verts[1]})
    assert list(db.infos) == ['obj_000001', 'obj_000005', 'obj_000012']
    for (label, row), (key, src) in zip(db.infos.items(), info.items()):
        assert set(row) == {'label', 'category', 'mesh_units', 'symmetries_discrete', 'symmetries_continuous', 'is_symmetric', 'diameter', 'diameter_m'}
        assert row['label'] == label == f'obj_{int(key):06d}' and row['mesh_units'] == 'mm' and row['category'] is None
        assert row['diameter'] == src['diameter'] and row['diameter_m'] == src['diameter'] * 0.001
        assert row['symmetries_discrete'] == src.get('symmetries_discrete', []) and row['symmetries_continuous'] == src.get('symmetries_continuous', [])
        assert row['is_symmetric'] == (key != '1')
    assert db.vertices['obj_000005'] is verts[1] and db.vertices['obj_000012'] is verts[2]
    m = MeshDataBase.from_models_info({7: dict(diameter=0.3)}, {7: verts[0]}, mesh_units='m')
    assert m.infos['obj_000007']['diameter_m'] == 0.3 and m.infos['obj_000007']['mesh_units'] == 'm'
    with pytest.raises(ValueError, match='Unit not supported'):
        MeshDataBase.from_models_info(info, {1: verts[0]}, mesh_units='cm')


def test_missing_diameters_need_the_device():
    """no diameter in the file: model_info is asked, and it has no CPU path"""
    from cosypose_amd import MeshDataBase, model_info
    from cosypose_amd._lib import CosyHipError
    with pytest.raises(CosyHipError, match='no CPU fallback'):
        MeshDataBase.from_models_info(None, {1: torch.zeros(4, 3)})
    with pytest.raises(CosyHipError, match='no CPU fallback'):
        model_info([torch.zeros(4, 3)])
    with pytest.raises(TypeError, match='float32 or float64'):
        model_info([torch.zeros(4, 3, dtype=torch.float16)])
    with pytest.raises(ValueError, match=r'model 1: vertices of shape \(0, 3\)'):
        model_info([torch.zeros(4, 3), torch.zeros(0, 3)])
    assert model_info([]) == [] and model_info.diameters([]).shape == (0,)


# ---- io_formats -----------------------------------------------------------------------------------------------------------------------------
def test_models_info_rows_round_trip():
    from cosypose_amd import MeshDataBase
    from cosypose_amd.io_formats import models_info_rows
    _, verts, _ = rows_and_verts()
    infos = [mr.info_ref(v) for v in verts[:3]]
    rows = models_info_rows(infos, [1, 5, 12], symmetries_discrete={5: [FLIP_Z]}, symmetries_continuous={12: [cont(2)], 1: []})
    assert list(rows) == ['1', '5', '12']
    assert set(rows['1']) == {'diameter', 'min_x', 'min_y', 'min_z', 'size_x', 'size_y', 'size_z'}
    assert set(rows['5']) - set(rows['1']) == {'symmetries_discrete'} and set(rows['12']) - set(rows['1']) == {'symmetries_continuous'}
    assert all(type(v) is float for v in rows['1'].values()) and rows['5']['symmetries_discrete'] == [[float(x) for x in FLIP_Z]]
    back = json.loads(json.dumps(rows))                                       # plain values: serialisable as they are, floats survive
    assert back == rows and all(back[k]['diameter'] == i['diameter'] for k, i in zip(('1', '5', '12'), infos))
    db = MeshDataBase.from_models_info(back, {1: verts[0], 5: verts[1], 12: verts[2]})
    assert [r['diameter'] for r in db.infos.values()] == [i['diameter'] for i in infos]
    assert [r['is_symmetric'] for r in db.infos.values()] == [False, True, True]
    assert db.batched(n_sym=8).symmetries.shape == (3, 8, 4, 4)


# ---- the package surface and the C ABI ----------------------------------------------------------------------------------------------------
def test_lazy_exports():
    import cosypose_amd
    from cosypose_amd import MeshDataBase, make_bop_symmetries, model_info
    assert MeshDataBase is cosypose_amd.mesh_db.MeshDataBase and make_bop_symmetries is cosypose_amd.mesh_db.make_bop_symmetries
    assert callable(model_info) and callable(cosypose_amd.model_info.model_info) and callable(cosypose_amd.model_info.diameters)


MODEL_SYMBOLS = ('cosy_model_info_workspace_bytes', 'cosy_model_info')


def test_c_abi_declares_exports_and_builds_the_model_entry_points():
    from cosypose_amd import _lib, model_info
    from cosypose_amd.build import build, SOURCES, FILE_FLAGS
    build()
    for name in MODEL_SYMBOLS:
        assert name in _lib.EXPORTS, name           # test_c_abi.py: EXPORTS, the header and the built library name the same entry points
    assert 'kernels_models.hip' in SOURCES and '-ffp-contract=off' in FILE_FLAGS['kernels_models.hip']
    src = (REPO / 'cosypose_amd' / 'csrc' / 'kernels_models.hip').read_text()
    assert int(re.search(r'constexpr int MI_TILE = (\d+);', src).group(1)) == model_info.TILE          # the tests size their models by it
    assert 'fma(' not in src


def test_argument_checks_run_on_the_host_before_any_launch():
    """COSY_EINVAL (-1) with the argument named, and n = 0 returns COSY_OK with null pointers: neither touches a device"""
    from cosypose_amd._lib import lib
    from cosypose_amd.model_info import TILE
    l = lib()
    P = 64          # a non-null, 16-byte aligned stand-in: every call below is refused (or returns) before a pointer is used
    off = np.array([0, 1, TILE + 1, 4 * TILE + 1], np.int64)                 # 1, TILE and 3 TILE vertices: 1 + 1 + 6 tiles
    h = off.ctypes.data
    assert l.cosy_model_info_workspace_bytes(h, 0) == 0 and l.cosy_model_info_workspace_bytes(None, 3) == 0
    need = l.cosy_model_info_workspace_bytes(h, 3)
    assert need == 32 + 8 * 16
    big = np.array([0, 2 ** 31 - 1], np.int64)                               # the largest model: 2^22 tile rows, 64-bit tile count
    nt = 2 ** 22
    assert l.cosy_model_info_workspace_bytes(big.ctypes.data, 1) == 16 + 16 * (nt * (nt + 1) // 2)

    def info(**kw):
        a = dict(verts=P, eb=4, off=P, host=h, n=3, out=P, ws=P, wb=need, st=None)
        a.update(kw)
        return l.cosy_model_info(*a.values())
    empty, back, neg, huge = (np.array(a, np.int64) for a in ([0, 1, 1, 5], [0, 4, 3, 9], [-1, 2, 3, 4], [0, 2 ** 31, 2 ** 31 + 1, 2 ** 31 + 2]))
    for bad, word in ((dict(n=-1), b'n=-1'), (dict(eb=2), b'elem_bytes=2'), (dict(verts=None), b'null verts'), (dict(off=None), b'null offsets'),
                      (dict(host=None), b'null host_offsets'), (dict(out=None), b'null out'), (dict(ws=None), b'null workspace'),
                      (dict(host=empty.ctypes.data), b'host_offsets'), (dict(host=back.ctypes.data), b'host_offsets'),
                      (dict(host=neg.ctypes.data), b'host_offsets'), (dict(host=huge.ctypes.data), b'2^31 - 1'),
                      (dict(verts=P + 2), b'verts not aligned'), (dict(verts=P + 4, eb=8), b'verts not aligned'), (dict(out=P + 4), b'out not 8-byte'),
                      (dict(wb=need - 1), b'workspace_bytes='), (dict(ws=P + 8), b'16-byte')):
        assert info(**bad) == -1 and word in l.cosy_last_error(), (bad, l.cosy_last_error())
    for a in (empty, back, neg, huge):
        assert l.cosy_model_info_workspace_bytes(a.ctypes.data, 3) == 0
    assert info(n=0, verts=None, off=None, host=None, out=None, ws=None, wb=0) == 0
