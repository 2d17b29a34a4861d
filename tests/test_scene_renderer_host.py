"""Host half of the scene renderer (cosypose_amd/scene_renderer.py, csrc/kernels_scene.hip) without a device: the C ABI's exports,
its refusals before any device work, the scratch sizing, render_scene's planning step, the device check -- and the yardstick of the GPU
tests held to itself: the twin composite (tests/scene_case.py) against the float64 composite on the base scene.
"""
import ctypes
import pathlib
import re

import numpy as np
import pytest

import scene_case as S

REPO = pathlib.Path(__file__).resolve().parent.parent
NAMES = ('cosy_render_scene_scratch_bytes', 'cosy_render_scene')
COSY_EINVAL = -1


def _lib():
    from cosypose_amd.build import build
    from cosypose_amd import _lib
    build()
    return _lib.lib()


def test_scene_entry_points_are_declared_exported_and_bound():
    from cosypose_amd import _lib
    from cosypose_amd.build import build
    build()
    header = re.sub(r'/\*.*?\*/', '', (REPO / 'include' / 'cosyhip.h').read_text(), flags=re.S)
    for name in NAMES:
        assert name in _lib.EXPORTS, name           # test_c_abi.py: EXPORTS, the header and the built library name the same entry points
    # the key split is stated in the header and admits what the issue asks for
    bits = int(re.search(r'#define COSY_SCENE_FACE_BITS (\d+)', header).group(1))
    assert (1 << bits) >= (1 << 20) and (1 << (32 - bits)) >= 256
    import cosypose_amd
    assert cosypose_amd.HipSceneRenderer.__name__ == 'HipSceneRenderer' and callable(cosypose_amd.scene_visibility)


def _call(lib, mesh=None, **over):
    """cosy_render_scene with good small arguments (dummy non-null device pointers: every call here is refused before they are used)"""
    from cosypose_amd._lib import MeshSet, Shade
    buf = (ctypes.c_int * 4096)()
    p = ctypes.addressof(buf)
    mf = dict(verts=p, colors=p, normals=p, uvs=None, tex=None, faces=p, n_faces=p, V=4, F=2, TH=0, TW=0)
    m = MeshSet(**dict(mf, **(mesh or {})))
    s = Shade(0.5, 0.5, 0.0, 1.0, (ctypes.c_float * 3)(0, 0, -1), 0, 0, 0)
    a = dict(obj_id=(ctypes.c_int * 2)(0, 0), view_id=(ctypes.c_int * 2)(0, 1), TCO=p, color=None, K=p, N=2, n_views=2, H=8, W=8,
             background=(ctypes.c_float * 3)(0, 0, 0), rgb=p, depth=None, mask=None, scratch=p)
    a.update(over)
    cast = lambda x: ctypes.cast(x, ctypes.c_void_p) if isinstance(x, ctypes.Array) else x
    return lib.cosy_render_scene(ctypes.byref(m), ctypes.byref(s), cast(a['obj_id']), cast(a['view_id']), a['TCO'], a['color'], a['K'], a['N'],
                                 a['n_views'], a['H'], a['W'], cast(a['background']), a['rgb'], a['depth'], a['mask'], None, None, None, None,
                                 a['scratch'], None)


def test_render_scene_refuses_bad_arguments_before_any_device_work():
    """No device here: a call that got as far as a launch or a copy would fail with COSY_EHIP, not with COSY_EINVAL and a message that
    names the argument."""
    lib = _lib()

    def refused(what, needle, **kw):
        rc = _call(lib, **kw)
        msg = lib.cosy_last_error().decode()
        print(f'  {what}: rc {rc}, "{msg}"')
        assert rc == COSY_EINVAL and needle in msg, (what, rc, msg)

    for n in ('TCO', 'K', 'rgb', 'scratch', 'obj_id', 'view_id', 'background'):
        refused(f'{n} = null', f'null {n}', **{n: None})
    for n in ('H', 'W'):
        for v in (0, -1):
            refused(f'{n} = {v}', f'{n}={v}', **{n: v})
    refused('N = -1', 'N=-1', N=-1)
    refused('N = 65536', 'N=65536', N=65536)
    refused('n_views = 65536', 'n_views=65536', n_views=65536)
    refused('n_views = -1', 'n_views=-1', n_views=-1)
    refused('view_id = 2 of 2', 'view_id 2', view_id=(ctypes.c_int * 2)(0, 2))
    refused('view_id = -1', 'view_id -1', view_id=(ctypes.c_int * 2)(-1, 0))
    refused('obj_id = -3', 'obj_id -3', obj_id=(ctypes.c_int * 2)(0, -3))
    header = (REPO / 'include' / 'cosyhip.h').read_text()
    face_bits = int(re.search(r'#define COSY_SCENE_FACE_BITS (\d+)', header).group(1))
    per_view = 1 << (32 - face_bits)
    n = per_view + 1                                                  # one instance more in view 1 than the key's slot bits admit
    refused('too many instances in a view', 'view 1 holds %d instances' % n, N=n + 1, obj_id=(ctypes.c_int * (n + 1))(),
            view_id=(ctypes.c_int * (n + 1))(0, *([1] * n)))
    refused('mesh->F beyond the face bits', 'mesh->F=%d' % ((1 << face_bits) + 1), mesh=dict(F=(1 << face_bits) + 1))
    refused('mesh->V = 0', 'V=0', mesh=dict(V=0))
    refused('null verts', 'null verts', mesh=dict(verts=None))


def test_scene_scratch_sizing():
    """Monotone in each argument, 0 for sizes the call rejects, and far below one z-buffer per row: N x H x W x 8 bytes is the cost
    the scene renderer removes."""
    lib = _lib()
    f = lib.cosy_render_scene_scratch_bytes
    base = dict(N=20, n_views=3, V=500, H=60, W=80)
    b0 = f(*base.values())
    assert b0 > 0
    for k in base:
        vals = [f(*dict(base, **{k: base[k] + d}).values()) for d in (0, 1, 7, 64)]
        assert vals == sorted(vals) and vals[-1] > vals[0], (k, vals)
    assert f(-1, 3, 500, 60, 80) == 0
    N, H, W, V = 200, 480, 640, 10000
    for n_views in (1, 8, 25):
        need = f(N, n_views, V, H, W)
        per_row = need - n_views * H * W * 8 - N * V * 12                 # what a row costs beyond its projected vertices
        print(f'  n_views {n_views}: {need / 2**20:.1f} MiB, of which per-row bit maps and tables {per_row / 2**20:.2f} MiB; '
              f'N z-buffers would be {N * H * W * 8 / 2**20:.0f} MiB')
        assert need < N * H * W * 8
        assert per_row <= N * H * W // 8 + 64 * N + 4 * n_views + 256     # the bit maps: N H W / 8 bytes plus O(N)


def test_plan_scene_rows_poses_and_resolution_groups():
    from cosypose_amd.scene_renderer import plan_scene
    rs = np.random.RandomState(0)
    from cosypose_amd.synthetic import _rigid_noise
    TWO = [_rigid_noise(rs, 1.0, 0.3) for _ in range(3)]
    TWC = [_rigid_noise(rs, 1.0, 0.5) for _ in range(4)]
    Ks = [np.array([[100. + i, 0, 40], [0, 101. + i, 30], [0, 0, 1]]) for i in range(4)]
    obj_infos = [dict(name='b', TWO=TWO[0]), dict(name='a', TWO=TWO[1], color=(1.0, 0.5, 0.25, 0.3)), dict(name='b', TWO=TWO[2].tolist())]
    res = [(80, 60), (32, 24), (60, 80), (24, 32)]                        # (w, h) or (h, w): the image is (min, max)
    cam_infos = [dict(K=Ks[i], TWC=TWC[i], resolution=res[i]) for i in range(4)]
    plans = plan_scene(obj_infos, cam_infos, label_to_id=dict(a=0, b=1))
    assert [p['resolution'] for p in plans] == [(60, 80), (24, 32)] and [p['cam_ids'] for p in plans] == [[0, 2], [1, 3]]
    for p in plans:
        assert p['obj_index'].tolist() == [0, 1, 2, 0, 1, 2] and p['view_ids'].tolist() == [0, 0, 0, 1, 1, 1] and p['view_ids'].dtype == np.int32
        assert p['labels'].tolist() == ['b', 'a', 'b'] * 2 and p['obj_ids'].tolist() == [1, 0, 1] * 2
        assert p['TCO'].dtype == np.float32 and p['K'].dtype == np.float32 and p['K'].shape == (2, 3, 3)
        for j, c in enumerate(p['cam_ids']):
            assert np.array_equal(p['K'][j], Ks[c].astype(np.float32))
            for o in range(3):
                want = (np.linalg.inv(TWC[c]) @ np.asarray(TWO[o], np.float64)).astype(np.float32)       # float64 product, rounded once
                assert np.array_equal(p['TCO'][j * 3 + o], want)
        assert p['colors'].shape == (6, 4) and (p['colors'][[0, 2, 3, 5], 3] < 0).all()
        assert np.array_equal(p['colors'][1], np.array([1.0, 0.5, 0.25, 0.3], np.float32)) and np.array_equal(p['colors'][4], p['colors'][1])
    assert plan_scene(obj_infos[:1], cam_infos[:1])[0]['colors'] is None
    assert plan_scene([], cam_infos[:1])[0]['TCO'].shape == (0, 4, 4)


def test_cpu_tensors_are_refused():
    import torch
    from cosypose_amd import HipSceneRenderer, scene_visibility, PandasTensorCollection
    from cosypose_amd._lib import CosyHipError
    import pandas as pd
    case = S.cases()['one_row']
    renderer = HipSceneRenderer(case.meshes())
    with pytest.raises(CosyHipError):
        renderer.render(case.row_labels, case.view, torch.from_numpy(case.TCO), torch.from_numpy(case.K), (case.H, case.W))
    with pytest.raises(CosyHipError):
        renderer.render_scene([dict(name=case.labels[0], TWO=np.eye(4))], [dict(K=case.K[0], TWC=np.eye(4), resolution=(80, 60))])
    objects = PandasTensorCollection(pd.DataFrame(dict(label=[case.labels[0]])), TWO=torch.eye(4)[None])
    cameras = PandasTensorCollection(pd.DataFrame(dict(view_id=[0])), TWC=torch.eye(4)[None], K=torch.from_numpy(case.K))
    with pytest.raises(CosyHipError):
        scene_visibility(renderer, objects, cameras, (case.H, case.W))


def test_twin_composite_vs_float64_composite_on_the_base_scene(oracle):
    """The yardstick of the GPU tests against the independent one: outside the exempt pixels (scene_case's rule) the twin composite's
    mask is the float64 composite's, and the exempt pixels stay within 2 % of each view's foreground -- by the references alone.  The
    base scene has real occlusion: in view 1 one instance keeps 10 of its 71 silhouette pixels."""
    case = S.cases()['base_60x80']
    tw = S.twin_composite(case, oracle)
    figs = S.compare_masks(case, tw['mask'], 'twin')
    assert all(f['foreground'] > 500 and f['near'] == 0 for f in figs)
    assert (int(tw['px_count_all'][7]), int(tw['px_count_visib'][7])) == (71, 10)
    assert (tw['px_count_visib'] <= tw['px_count_all']).all() and (tw['px_count_visib'] < tw['px_count_all']).sum() >= 10
    # every winner lies inside its row's silhouette and box
    for r in range(case.N):
        won = tw['mask'][case.view[r]] == r
        assert not (won & ~tw['silhouettes'][r]).any()
        if won.any():
            bo, bv = tw['bbox_obj'][r], tw['bbox_visib'][r]
            assert bo[0] <= bv[0] and bo[1] <= bv[1] and bv[2] <= bo[2] and bv[3] <= bo[3]
