"""The scene renderer on the device -- HipSceneRenderer.render / render_scene, scene_visibility, csrc/kernels_scene.hip -- against
the twin composite (bit for bit) and the float64 composite (mask, under the exemption rule) of tests/scene_case.py, on the small
case matrix there: every case is a few rows in at most four 60x80 or 45x61 views.
"""
import numpy as np
import pandas as pd
import pytest
import torch

import scene_case as S

pytestmark = pytest.mark.gpu
STAT_KEYS = ('px_count_all', 'px_count_visib', 'bbox_obj', 'bbox_visib', 'visib_fract')
OUT_KEYS = ('rgb', 'depth', 'mask') + STAT_KEYS


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to('cuda', dtype).contiguous()


def _renderer(case, meshes=None):
    from cosypose_amd import HipSceneRenderer
    return HipSceneRenderer((meshes or case.meshes()).cuda(), background_color=case.background, shading=case.shading_name)


def _render(case, renderer, rows=None, views=None):
    """the case (or some of its rows, in the given order; or some of its views, renumbered) with every output"""
    rows = np.arange(case.N) if rows is None else np.asarray(rows)
    view, K = case.view[rows], case.K
    if views is not None:
        renumber = {v: i for i, v in enumerate(views)}
        view, K = np.array([renumber[v] for v in view], np.int32), case.K[list(views)]
    colors = None if case.row_colors is None else dev(case.row_colors[rows])
    return renderer.render(case.row_labels[rows], view, dev(case.TCO[rows]), dev(K), (case.H, case.W), colors=colors, render_depth=True,
                           render_mask=True, stats=True)


_GPU = {}


def _gpu_case(name):
    """(case, renderer, outputs on the device) of one render of the case, cached for the module"""
    if name not in _GPU:
        case = S.cases()[name]
        renderer = _renderer(case)
        out = _render(case, renderer)
        torch.cuda.synchronize()
        _GPU[name] = (case, renderer, out)
    return _GPU[name]


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b, keys=OUT_KEYS):
    return [k for k in keys if not torch.equal(_bits(a[k]), _bits(b[k]))]


@pytest.mark.parametrize('name', S.CASE_NAMES)
def test_kernel_equals_the_twin_composite(oracle, name):
    """mask, depth bits, both pixel counts and both boxes equal the twin composite exactly; visib_fract is the float32 quotient; rgb is
    bit-equal, except with a highlight (powf: specular > 0), which gets the allowance test_raster_kernels._equal_to_twin grants the batch
    renderer: at most 1/255 on fewer than 1e-3 of the values."""
    case, _, out = _gpu_case(name)
    want = S.twin_composite(case, oracle)
    got = {k: out[k].cpu().numpy() for k in OUT_KEYS}
    assert got['rgb'].shape == (case.n_views, 3, case.H, case.W) and got['mask'].dtype == np.int32 and got['px_count_all'].dtype == np.int32
    assert np.array_equal(got['mask'], want['mask']), (name, int((got['mask'] != want['mask']).sum()))
    assert np.array_equal(got['depth'].view(np.uint32), want['depth'].view(np.uint32)), (name, int((got['depth'] != want['depth']).sum()))
    if case.shading['specular'] > 0:
        diff = np.abs(got['rgb'] - want['rgb'])
        assert diff.max() <= 1 / 255 + 1e-6 and (diff > 1e-6).mean() < 1e-3, (name, float(diff.max()), float((diff > 1e-6).mean()))
    else:
        assert np.array_equal(got['rgb'].view(np.uint32), want['rgb'].view(np.uint32)), (name, float(np.abs(got['rgb'] - want['rgb']).max()))
    for k in ('px_count_all', 'px_count_visib', 'bbox_obj', 'bbox_visib'):
        assert np.array_equal(got[k], want[k]), (name, k, got[k].tolist(), want[k].tolist())
    assert np.array_equal(got['visib_fract'].view(np.uint32), want['visib_fract'].view(np.uint32)), (name, got['visib_fract'], want['visib_fract'])
    bg = got['mask'] < 0
    assert (got['depth'][bg] == 0).all() and all((got['rgb'][:, k][bg] == case.background32[k]).all() for k in range(3))


@pytest.mark.parametrize('name', S.CASE_NAMES)
def test_kernel_mask_vs_float64_composite(name):
    case, _, out = _gpu_case(name)
    S.compare_masks(case, out['mask'].cpu().numpy(), 'kernel')


@pytest.mark.parametrize('name', S.CASE_NAMES)
def test_rerun_view_split_and_row_permutation(name):
    """A second run is bit-identical; each view rendered in a call of its own equals its slice of the joint call (and its rows'
    statistics); a permutation of the rows leaves rgb and depth bit-identical, maps the mask through the permutation (outside the
    tie case, where the row that now comes first wins) and permutes the silhouette statistics."""
    case, renderer, out = _gpu_case(name)
    again = _render(case, renderer)
    assert _same(again, out) == []
    for v in range(case.n_views):
        rows = np.flatnonzero(case.view == v)
        one = _render(case, renderer, rows=rows, views=[v])
        assert torch.equal(_bits(one['rgb'][0]), _bits(out['rgb'][v])) and torch.equal(_bits(one['depth'][0]), _bits(out['depth'][v])), (name, v)
        m = out['mask'][v].cpu().numpy()
        want = np.where(m >= 0, np.searchsorted(rows, np.maximum(m, 0)), -1)             # row index -> rank within the view
        assert np.array_equal(one['mask'][0].cpu().numpy(), want), (name, v)
        idx = torch.as_tensor(rows, device='cuda')
        assert all(torch.equal(_bits(one[k]), _bits(out[k][idx])) for k in STAT_KEYS), (name, v)
    perm = np.random.RandomState(9).permutation(case.N)
    p = _render(case, renderer, rows=perm)
    assert _same(p, out, ('rgb', 'depth')) == [], name
    idx = torch.as_tensor(perm, device='cuda')
    assert torch.equal(p['px_count_all'], out['px_count_all'][idx]) and torch.equal(p['bbox_obj'], out['bbox_obj'][idx])
    if not case.tie:
        m = out['mask'].cpu().numpy()
        inv = np.argsort(perm)                                                           # old row -> new row
        assert np.array_equal(p['mask'].cpu().numpy(), np.where(m >= 0, inv[np.maximum(m, 0)], -1)), name
        assert all(torch.equal(_bits(p[k]), _bits(out[k][idx])) for k in STAT_KEYS), name


def test_one_row_equals_the_batch_renderer():
    from cosypose_amd import HipBatchRenderer
    case, renderer, out = _gpu_case('one_row')
    batch = HipBatchRenderer(renderer.meshes, shading='flat')
    rgb, depth = batch.render([dict(name=l) for l in case.row_labels], dev(case.TCO), dev(case.K), resolution=(case.H, case.W), render_depth=True)
    assert bool((depth > 0).any())
    assert torch.equal(_bits(out['rgb']), _bits(rgb)) and torch.equal(_bits(out['depth']), _bits(depth))


def test_statistics_of_the_edge_cases():
    """What the cases were built to show (the twin composite says the same: test_kernel_equals_the_twin_composite)."""
    n = lambda name, k: _gpu_case(name)[2][k].cpu().numpy()
    a, v = n('same_pose_twice', 'px_count_all'), n('same_pose_twice', 'px_count_visib')
    assert a[0] == a[1] > 0 and v[1] == 0 and v[0] > 0              # the first row wins every pixel of the pair
    assert not bool((_gpu_case('same_pose_twice')[2]['mask'] == 1).any())
    a, v = n('behind_box', 'px_count_all'), n('behind_box', 'px_count_visib')
    assert a[0] > 0 and v[0] == 0 and a[3] > 0 and v[3] == 0        # wholly behind the box, whichever comes first in the call
    assert (n('behind_box', 'bbox_visib')[[0, 3]] == -1).all() and (n('behind_box', 'bbox_obj')[[0, 3]] >= 0).all()
    a = n('outside_frame', 'px_count_all')
    assert a[0] == 0 and a[2] == 0 and a[1] > 0
    assert (n('outside_frame', 'bbox_obj')[[0, 2]] == -1).all() and (n('outside_frame', 'bbox_visib')[[0, 2]] == -1).all()
    assert n('outside_frame', 'visib_fract')[0] == 0


def test_non_finite_row_or_view_draws_nothing_and_leaves_the_rest():
    base, renderer, out = _gpu_case('base_60x80')
    # NaN in one row's TCO: the row counts 0, everything else is the call without the row
    case, _, bad = _gpu_case('nan_in_TCO')
    r = 11
    assert int(bad['px_count_all'][r]) == 0 and int(bad['px_count_visib'][r]) == 0 and not bool((bad['mask'] == r).any())
    keep = np.array([i for i in range(base.N) if i != r])
    without = _render(base, renderer, rows=keep)
    assert _same(bad, without, ('rgb', 'depth')) == []
    m = without['mask'].cpu().numpy()
    assert np.array_equal(bad['mask'].cpu().numpy(), np.where(m >= 0, keep[np.maximum(m, 0)], -1))
    idx = torch.as_tensor(keep, device='cuda')
    assert all(torch.equal(_bits(bad[k][idx]), _bits(without[k])) for k in STAT_KEYS)
    # NaN in one view's K: that view is background, the others are bit-identical
    case, _, bad = _gpu_case('nan_in_K')
    assert bool((bad['mask'][1] == -1).all()) and bool((bad['depth'][1] == 0).all()) and bool((bad['rgb'][1] == 0).all())
    assert bool((out['mask'][1] >= 0).any())
    for v in (0, 2):
        assert all(torch.equal(_bits(bad[k][v]), _bits(out[k][v])) for k in ('rgb', 'depth', 'mask'))
    rows = torch.as_tensor(np.flatnonzero(base.view != 1), device='cuda')
    assert all(torch.equal(_bits(bad[k][rows]), _bits(out[k][rows])) for k in STAT_KEYS)
    assert int(bad['px_count_all'][base.view == 1].sum()) == 0


def test_colour_override_equals_uniformly_coloured_meshes():
    """A row drawn with colors[r] = (rgb, alpha >= 0) is the row drawn from a RenderMeshes whose vertex colours are uniformly that rgb;
    alpha < 0 keeps the mesh's own colours; the alpha value changes nothing."""
    case, renderer, out = _gpu_case('colour_override')
    meshes, obj = case.flat_meshes()
    flat = _renderer(case, meshes)
    want = flat.render(meshes.labels[obj], case.view, dev(case.TCO), dev(case.K), (case.H, case.W), render_depth=True, render_mask=True, stats=True)
    assert _same(out, want) == []
    plain = _gpu_case('base_60x80')[2]
    assert _same(out, plain, ('depth', 'mask') + STAT_KEYS) == [] and _same(out, plain, ('rgb',)) == ['rgb']
    over = np.isin(plain['mask'].cpu().numpy(), np.flatnonzero(case.row_colors[:, 3] >= 0))
    same = (out['rgb'] == plain['rgb']).all(1).cpu().numpy()
    assert same[~over].all() and not same[over].all()
    col = case.row_colors.copy(); col[col[:, 3] >= 0, 3] = 0.7
    other = renderer.render(case.row_labels, case.view, dev(case.TCO), dev(case.K), (case.H, case.W), colors=dev(col))
    assert torch.equal(_bits(other['rgb']), _bits(out['rgb'])) and other['depth'] is None and other['mask'] is None and other['visib_fract'] is None


def test_empty_call_is_background():
    case, renderer, _ = _gpu_case('background')
    out = renderer.render([], np.zeros(0, np.int32), torch.zeros(0, 4, 4, device='cuda'), dev(case.K), (case.H, case.W), render_depth=True,
                          render_mask=True, stats=True)
    assert bool((out['mask'] == -1).all()) and bool((out['depth'] == 0).all()) and out['px_count_all'].shape == (0,) and out['bbox_obj'].shape == (0, 4)
    assert bool((out['rgb'] == dev(case.background32)[None, :, None, None]).all())


def test_render_scene_has_the_reference_shape(oracle):
    """One dict per camera, in camera order: rgb (H,W,3) uint8 = floor(255 rgb + 0.5) of .render, mask (H,W) int32 = index into
    obj_infos (-1 background), depth (H,W) float32 only when asked; cameras of two resolutions are served by one launch each."""
    case, renderer, out = _gpu_case('base_60x80')
    TWO, TWC = S.base_world()
    obj_infos = [dict(name=case.labels[o], TWO=TWO[i]) for i, o in enumerate(S.BASE_OBJECTS)]
    K45 = S.cases()['base_45x61'].K
    cam_infos = [dict(K=case.K[0], TWC=TWC[0], resolution=(80, 60)), dict(K=K45[1], TWC=TWC[1], resolution=(45, 61)),
                 dict(K=case.K[2], TWC=TWC[2], resolution=(60, 80)), dict(K=case.K[1], TWC=TWC[1], resolution=(80, 60))]
    obs = renderer.render_scene(obj_infos, cam_infos, render_depth=True)
    assert isinstance(obs, list) and len(obs) == 4
    small = _gpu_case('base_45x61')[2]
    for ob, (src, v) in zip(obs, ((out, 0), (small, 1), (out, 2), (out, 1))):
        H, W = src['rgb'].shape[2:]
        assert set(ob) == {'rgb', 'mask', 'depth'}
        assert ob['rgb'].shape == (H, W, 3) and ob['rgb'].dtype == np.uint8 and ob['mask'].shape == (H, W) and ob['mask'].dtype == np.int32
        assert ob['depth'].shape == (H, W) and ob['depth'].dtype == np.float32
        want = torch.floor(src['rgb'][v] * 255.0 + 0.5).to(torch.uint8).permute(1, 2, 0).cpu().numpy()
        assert np.array_equal(ob['rgb'], want)
        m = src['mask'][v].cpu().numpy()
        assert np.array_equal(ob['mask'], np.where(m >= 0, m - 7 * v, -1)) and ob['mask'].max() <= 6
        assert np.array_equal(ob['depth'].view(np.uint32), src['depth'][v].cpu().numpy().view(np.uint32))
    assert set(renderer.render_scene(obj_infos, cam_infos[:1])[0]) == {'rgb', 'mask'}
    # a colour in obj_infos is the colour override of every row of that object
    red = [dict(o, color=(1.0, 0.0, 0.0, 1.0)) if i == 1 else o for i, o in enumerate(obj_infos)]
    ob = renderer.render_scene(red, cam_infos[:1])[0]
    px = ob['mask'] == 1
    assert px.any() and (ob['rgb'][px][:, 1:] == 0).all() and (ob['rgb'][px][:, 0] > 0).all() and np.array_equal(ob['mask'], obs[0]['mask'])


def test_scene_visibility_follows_reproject_scene():
    from cosypose_amd import scene_visibility, PandasTensorCollection, MultiviewScenePredictor
    case, renderer, out = _gpu_case('base_60x80')
    TWO, TWC = S.base_world()
    labels = case.labels[list(S.BASE_OBJECTS)]
    objects = PandasTensorCollection(pd.DataFrame(dict(label=labels, obj_id=100 + np.arange(7), score=np.ones(7), view_group=np.zeros(7, int))),
                                     TWO=dev(TWO, torch.float64))
    cameras = PandasTensorCollection(pd.DataFrame(dict(view_id=[10, 13, 16], scene_id=[1, 1, 1], batch_im_id=[0, 1, 2])), TWC=dev(TWC, torch.float64),
                                     K=dev(case.K, torch.float64))
    vis = scene_visibility(renderer, objects, cameras, (case.H, case.W))
    rep = MultiviewScenePredictor(None).reproject_scene(objects, cameras)
    assert len(vis) == 21 and list(vis.infos.columns) == ['view_id', 'label', 'obj_id', 'px_count_all', 'px_count_visib', 'visib_fract']
    for k in ('view_id', 'label', 'obj_id'):
        assert np.array_equal(vis.infos[k].values, rep.infos[k].values), k
    assert torch.equal(vis.poses, rep.poses)
    # rows are object-major here and view-major in the case: row o * 3 + v is the case's row v * 7 + o
    to_case = np.array([v * 7 + o for o in range(7) for v in range(3)])
    assert np.abs(vis.poses.float().cpu().numpy() - case.TCO[to_case]).max() < 1e-6
    want = renderer.render(np.repeat(labels, 3), np.tile(np.arange(3), 7), vis.poses, dev(case.K), (case.H, case.W), stats=True)
    for k in ('px_count_all', 'px_count_visib', 'visib_fract'):
        assert np.array_equal(vis.infos[k].values, want[k].cpu().numpy()), k
    assert torch.equal(vis.bboxes, want['bbox_visib']) and torch.equal(vis.bboxes_obj, want['bbox_obj'])
    idx = torch.as_tensor(to_case, device='cuda')
    assert (vis.infos['px_count_all'].values > 0).all() and np.abs(vis.infos['px_count_all'].values - out['px_count_all'][idx].cpu().numpy()).max() <= 2
    assert (vis.infos['visib_fract'] < 0.2).sum() >= 1 and (vis.infos['visib_fract'] == 1).sum() >= 3


def test_side_stream_while_the_default_stream_is_busy():
    """The call on a side stream, with the default stream kept busy by other renders of the same renderer, gives the default stream's
    bits: scratch is per stream (the batch renderer once shared one)."""
    case, renderer, out = _gpu_case('base_60x80')
    other = S.cases()['coarse_over_fine']
    busy_renderer = _renderer(other)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    results = []
    for _ in range(3):
        for _ in range(4):
            _render(case, renderer, rows=np.random.RandomState(3).permutation(case.N))        # default stream: same renderer, other row order
            _render(other, busy_renderer)
        with torch.cuda.stream(side):
            results.append(_render(case, renderer))
    torch.cuda.synchronize()
    assert len(renderer._scratch) >= 2
    for r in results:
        assert _same(r, out) == []
