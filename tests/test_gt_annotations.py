"""BOP ground-truth annotations on the GPU (cosypose_amd/gt_annotations.py, csrc/kernels_gt.hip) against the numpy twin of
tests/gt_ref.py.  The contract is DESIGN.md section 19 (the BOP toolkit's published definition restated; not a recording of the toolkit).

Yardsticks (every test prints its figures before it asserts):
  (A) D_gt_large is the package's own full-frame render at (3H, 3W) under K' (HipBatchRenderer.render(..., render_depth=True)); on it the
      float32 twin gives counts, boxes, id_in_segm, the composite and the dense masks, all of which must be EQUAL;
  (B) the float64 twin decides the same pixels outside the undecided ones (dist_gt - t within 13 u max(dist) of delta), and those are
      at most 2 % of the pixels inside the masks;
  (C) equal output in chunks, from run to run and on another stream; N = 0; non-finite poses and K rows; argument checks;
  (D) annotate_gt feeds BopScoreMeter.add and DetectionMeter.add: the valid ground truth is what the twin's fractions give.
"""
import numpy as np
import pandas as pd
import pytest
import torch

import bop_ref as br
import gt_ref as gr
import raster_ref

pytestmark = pytest.mark.gpu

HW = (48, 64)
N_VIEWS = 3
STRIP = 2048                      # GT_STRIP of kernels_gt.hip
INT_KEYS = ('px_count_all', 'px_count_valid', 'px_count_visib', 'bbox_obj', 'bbox_visib', 'id_in_segm')
ALL_KEYS = INT_KEYS + ('visib_fract', 'mask_visib_all', 'mask', 'mask_visib')


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def mesh_lists():
    """a 2-triangle square, a box and a bumpy sphere of 288 faces -> labels, verts, faces"""
    from cosypose_amd import synthetic as syn
    sq = np.array([[-0.04, -0.04, 0], [0.04, -0.04, 0], [0.04, 0.04, 0], [-0.04, 0.04, 0]], np.float32)
    box_v, box_f = raster_ref._box(0.05, 0.04, 0.03)
    sv, sf, _ = syn.make_render_meshes(5, 1, 10, 16)
    assert len(sf[0]) == 288
    return ['square', 'box', 'sphere'], [sq, box_v, sv[0]], [np.array([[0, 1, 2], [0, 2, 3]], np.int32), box_f, sf[0]]


@pytest.fixture(scope='module')
def models():
    from cosypose_amd import BopModels
    return BopModels(*mesh_lists()).cuda()


def canvas_K(K):
    H, W = HW
    Kc = K.copy()
    Kc[:, 0, 2] = Kc[:, 0, 2] + np.float32(W)
    Kc[:, 1, 2] = Kc[:, 1, 2] + np.float32(H)
    return Kc


def canvas_frames(models, obj, view, TCO, K):
    """(N,3H,3W) numpy: every instance alone on the canvas, the package's full-frame render under K'"""
    from cosypose_amd import HipBatchRenderer
    H, W = HW
    if len(obj) == 0:
        return np.zeros((0, 3 * H, 3 * W), np.float32)
    infos = [dict(name=models.labels[o]) for o in obj]
    _, depth = HipBatchRenderer(models.meshes).render(infos, dev(TCO), dev(canvas_K(K)[np.asarray(view)]), resolution=(3 * H, 3 * W), render_depth=True)
    return depth.cpu().numpy()


def pose_at(K, u, v, z, R=None):
    """a pose whose origin projects to frame coordinate (u, v) at depth z"""
    T = np.eye(4, dtype=np.float64)
    if R is not None:
        T[:3, :3] = R
    T[:3, 3] = [(u - K[0, 2]) * z / K[0, 0], (v - K[1, 2]) * z / K[1, 1], z]
    return T.astype(np.float32)


def sensor_depth(D_gt, rs, wall=2.0, noise=0.004):
    """a measured frame: the nearest instance, a wall behind, millimetre noise, missing pixels, an occluding bar and two NaN pixels"""
    d = np.where(D_gt > 0, D_gt, np.inf).min(0) if len(D_gt) else np.full(HW, np.inf)
    d = np.where(np.isfinite(d), d, wall).astype(np.float32)
    d = (d + rs.uniform(-noise, noise, d.shape)).astype(np.float32)
    d[rs.uniform(size=d.shape) < 0.03] = 0.0
    d[:, 40:43] = 0.2
    d[10, 10] = d[30, 31] = np.nan
    return d


def make_scene(render):
    """40 instances in views 0 and 2 of 3 (view 1 holds none), rows interleaved; the first ten reach the paths the issue names, in front
    of the thirty random ones.  render(obj, view, TCO, K) -> (N,3H,3W) canvas depths; they and the twins' results are computed once."""
    H, W = HW
    rs = np.random.RandomState(11)
    K = br.make_K(N_VIEWS, H, W)
    K[2, 0, 2] -= 2.5; K[2, 1, 1] *= 1.1
    N = 40
    R = br.rand_pose(rs, N)[:, :3, :3]
    view = np.where(np.arange(N) % 3 == 1, 2, 0)                       # 0 2 0 0 2 0 ...: interleaved
    obj = rs.randint(0, 3, N)
    k = lambda n: K[view[n]]
    poses = [pose_at(k(n), rs.uniform(0.1, 0.9) * W, rs.uniform(0.1, 0.9) * H, rs.uniform(1.0, 1.5), R[n]) for n in range(N)]
    obj[0] = 2; poses[0] = pose_at(k(0), W / 2, H / 2, 0.3, R[0])               # close: a window of several strips
    obj[1] = 2; poses[1] = pose_at(k(1), -W + 0.0, -H + 0.0, 100.0, R[1])        # far, at the canvas corner: a 1-pixel window, nothing drawn
    obj[2] = 2; poses[2] = pose_at(k(2), -W + 0.5, -H + 0.5, 100.0, R[1])        # on the centre of canvas pixel (0, 0): one pixel drawn, off the frame
    obj[3] = 1; poses[3] = pose_at(k(3), W / 2, H / 2, -0.5, R[3])              # behind the near plane: an empty box
    obj[4] = 2; poses[4] = pose_at(k(4), 0.0, H / 2, 0.6, R[4])                 # cut by the frame's left edge
    obj[5] = 2; poses[5] = pose_at(k(5), -30.0, H / 2, 0.9, R[5])               # wholly outside the frame, on the canvas
    obj[6] = 1; poses[6] = pose_at(k(6), 40.0 * W, H / 2, 0.9, R[6])            # off the canvas
    obj[7] = 1; poses[7] = pose_at(k(7), W - 1.0, H + 3.0, 0.6, R[7])           # cut by a corner
    obj[8] = 0; poses[8] = pose_at(k(8), W / 2, H / 2, 1.0, 2 * np.eye(3))      # the fronto-parallel square, 17 pixels wide ...
    obj[9] = 0; poses[9] = pose_at(k(9), W / 2 + 3, H / 2, 1.01, 2 * np.eye(3))  # ... and one 1 cm behind it, shifted: both visible where they overlap
    assert view[8] == view[9] == 0
    TCO = np.stack(poses)
    D_large = render(obj, view, TCO, K)
    crop = D_large[:, H:2 * H, W:2 * W]
    depth = np.stack([sensor_depth(crop[view == v], np.random.RandomState(20 + v)) for v in range(N_VIEWS)])
    both = (crop[8] > 0) & (crop[9] > 0)
    depth[0][both] = crop[8][both]                                      # the sensor sees the nearer square exactly
    ys, xs = np.nonzero(crop[4])
    depth[view[4], ys[len(ys) // 2], xs[len(ys) // 2]] = np.nan         # a NaN sensor value inside a mask
    ref32 = [gr.gt_info_ref(D_large[n], depth[view[n]], K[view[n]]) for n in range(N)]
    ref64 = [gr.gt_info_ref(D_large[n], depth[view[n]], K[view[n]], exact=True) for n in range(N)]
    return dict(TCO=TCO, obj=obj, view=view, K=K, depth=depth, D_large=D_large, ref32=ref32, ref64=ref64)


@pytest.fixture(scope='module')
def scene(models):
    return make_scene(lambda obj, view, TCO, K: canvas_frames(models, obj, view, TCO, K))


def run(models, s, sel=None, **kw):
    from cosypose_amd import gt_info
    sel = np.arange(len(s['obj'])) if sel is None else np.asarray(sel, dtype=np.int64)
    out = gt_info(dev(kw.pop('TCO', s['TCO'])[sel]), s['obj'][sel].astype(np.int32), s['view'][sel].astype(np.int32), dev(kw.pop('K', s['K'])),
                  dev(s['depth']), models, delta=gr.DELTA, dense_masks=kw.pop('dense_masks', True), **kw)
    torch.cuda.synchronize()
    return out


def same(a, b, keys=ALL_KEYS):
    return all(torch.equal(a[k], b[k]) for k in keys if k in a or k in b)


@pytest.fixture(scope='module')
def result(models, scene):
    return run(models, scene)


# ---- (A), (B) against the twins ----------------------------------------------------------------------------------------------------------------
def test_everything_equals_the_float32_twin(models, scene, result):
    s, out = scene, result
    N = len(s['obj'])
    got = {k: out[k].cpu().numpy() for k in out}
    assert all(got[k].dtype == np.int32 for k in INT_KEYS) and got['visib_fract'].dtype == np.float64 and got['mask_visib_all'].dtype == np.uint8
    assert got['mask'].dtype == bool and got['mask'].shape == (N,) + HW and got['mask_visib_all'].shape == (N_VIEWS,) + HW
    for n, r in enumerate(s['ref32']):
        mine = dict(px_count_all=int(got['px_count_all'][n]), px_count_valid=int(got['px_count_valid'][n]), px_count_visib=int(got['px_count_visib'][n]),
                    bbox_obj=got['bbox_obj'][n].tolist(), bbox_visib=got['bbox_visib'][n].tolist(), visib_fract=float(got['visib_fract'][n]))
        print(n, 'obj', s['obj'][n], 'view', s['view'][n], mine)
        for k, v in mine.items():
            assert v == r[k], (n, k, v, r[k])
        assert np.array_equal(got['mask'][n], r['mask']) and np.array_equal(got['mask_visib'][n], r['mask_visib']), n
    assert np.array_equal(got['id_in_segm'], gr.id_in_segm_ref(s['view']))
    want_all = gr.composite_ref(np.stack([r['mask_visib'] for r in s['ref32']]), s['view'], N_VIEWS)
    assert np.array_equal(got['mask_visib_all'], want_all)
    assert not got['mask_visib_all'][1].any() and got['mask_visib_all'][0].any() and got['mask_visib_all'][2].any()         # the view without instances
    # the composite without the dense masks is the same
    assert same(run(models, s, dense_masks=False), out, INT_KEYS + ('visib_fract', 'mask_visib_all'))


def check_paths(s, boxes):
    """the scene holds what it was built for; boxes (N,4): the canvas boxes of the instances"""
    H, W = HW
    r = s['ref32']
    size = np.maximum(boxes[:, 2] - boxes[:, 0] + 1, 0) * np.maximum(boxes[:, 3] - boxes[:, 1] + 1, 0)
    print('window sizes', size.tolist())
    assert size[0] > 2 * STRIP and r[0]['px_count_all'] > STRIP                                  # several strips
    assert boxes[1].tolist() == [0, 0, 0, 0] and r[1]['px_count_all'] == 0                          # a 1-pixel window
    assert size[2] == 4 and r[2]['px_count_all'] == 1 and r[2]['px_count_visib'] == 0 and r[2]['bbox_obj'] == [-1] * 4
    assert size[3] == 0 and r[3]['px_count_all'] == 0 and r[3]['visib_fract'] == 0.0               # behind the near plane
    assert r[4]['bbox_obj'][0] < 0 < r[4]['px_count_visib'] and r[4]['mask'].sum() < r[4]['px_count_all'] and r[4]['bbox_visib'][0] == 0
    assert r[5]['px_count_all'] > 50 and r[5]['px_count_valid'] == 0 and not r[5]['mask'].any() and r[5]['bbox_obj'] == [-1] * 4
    assert size[6] == 0
    assert r[7]['bbox_obj'][1] + r[7]['bbox_obj'][3] >= H and r[7]['bbox_obj'][0] + r[7]['bbox_obj'][2] >= W - 1
    both = r[8]['mask_visib'] & r[9]['mask_visib']
    assert both.sum() > 50
    fr = np.array([x['visib_fract'] for x in r])
    print('visib_fract', np.round(fr, 3).tolist())
    assert (fr == 0).sum() >= 4 and (fr > 0.9).sum() >= 1 and ((fr > 0.05) & (fr < 0.9)).sum() >= 5     # hidden, seen and in between
    assert any(0 < x['px_count_valid'] < x['mask'].sum() for x in r)                                # missing sensor pixels inside a mask
    nan_at = np.argwhere(np.isnan(s['depth']))
    assert any(r[n]['mask'][y, x] and not r[n]['mask_visib'][y, x] for v, y, x in nan_at for n in np.flatnonzero(s['view'] == v))
    return both


def test_the_scene_reaches_every_path(models, scene, result):
    from cosypose_amd import bop_errors as be
    from cosypose_amd.gt_annotations import canvas_K as canvas_K_dev
    s = scene
    H, W = HW
    Kd = dev(s['K'])
    boxes = be.instance_boxes(dev(s['TCO']), dev(s['obj'].astype(np.int32)), dev(s['view'].astype(np.int32)), canvas_K_dev(Kd, HW), models,
                              (3 * H, 3 * W)).cpu().numpy().astype(np.int64)
    assert np.array_equal(canvas_K_dev(Kd, HW).cpu().numpy(), canvas_K(s['K']))
    both = check_paths(s, boxes)
    ids = result['id_in_segm'].cpu().numpy()
    assert ids[9] > ids[8] and (result['mask_visib_all'][0].cpu().numpy()[both] >= ids[9]).all()


def test_float64_twin_agrees_outside_the_undecided_pixels(scene, result):
    got = result['mask_visib'].cpu().numpy()
    undecided = inside = 0
    for n, r in enumerate(scene['ref64']):
        u = r['undecided']
        undecided += int(u.sum()); inside += int(r['mask'].sum())
        assert np.array_equal(got[n][~u], r['mask_visib'][~u]), n
        lo = int((r['mask_visib'] & ~u).sum())
        assert lo <= int(result['px_count_visib'][n]) <= lo + int(u.sum()), n
        assert int(result['px_count_all'][n]) == r['px_count_all'] and int(result['px_count_valid'][n]) == r['px_count_valid']
    print(f'undecided pixels: {undecided} of {inside} inside the masks = {100.0 * undecided / max(inside, 1):.4f} %')
    assert inside > 3000 and undecided <= 0.02 * inside


def test_hand_cases_on_the_device():
    """the squares of gt_ref.hand_cases drawn by the two-triangle mesh: the twin's hand values through the kernels"""
    from cosypose_amd import BopModels, gt_info
    v = np.array([[-0.04, -0.04, 0], [0.04, -0.04, 0], [0.04, 0.04, 0], [-0.04, 0.04, 0]], np.float32)
    sq = BopModels(['square'], [v], [np.array([[0, 1, 2], [0, 2, 3]], np.int32)]).cuda()
    at = {'half left of the frame': 0.0, 'outside the frame, on the canvas': -32.0}
    for name, D_large, D_test, want in gr.hand_cases():
        T = pose_at(br.HAND_K, at.get(name, 24.0), 24.0, 1.0)
        out = gt_info(dev(T[None]), [0], [0], dev(br.HAND_K[None]), dev(D_test[None]), sq, delta=gr.DELTA)
        got = {k: out[k][0].tolist() for k in want}
        print(name, got)
        assert got == want, name


# ---- (C) chunks, determinism, streams, edges -----------------------------------------------------------------------------------------------------
def test_chunks_give_the_same_output(models, scene, result):
    from cosypose_amd import bop_errors as be
    from cosypose_amd.gt_annotations import canvas_K as canvas_K_dev, plan_chunks
    s = scene
    H, W = HW
    boxes = be.instance_boxes(dev(s['TCO']), dev(s['obj'].astype(np.int32)), dev(s['view'].astype(np.int32)), canvas_K_dev(dev(s['K']), HW), models,
                              (3 * H, 3 * W)).cpu().numpy().astype(np.int64)
    size = np.maximum(boxes[:, 2] - boxes[:, 0] + 1, 0) * np.maximum(boxes[:, 3] - boxes[:, 1] + 1, 0)
    cap = int(size.max()) * 4                                            # the tightest cap that still holds every instance
    chunks = plan_chunks(boxes, cap // 4)
    print('cap', cap, 'bytes:', len(chunks), 'chunks of', [c['n_pixels'] for c in chunks], 'pixels; unlimited:', int(size.sum()))
    assert len(chunks) >= 3
    assert same(run(models, s, max_workspace_bytes=cap), result)
    with pytest.raises(ValueError, match='alone needs'):
        run(models, s, max_workspace_bytes=cap - 4)


def test_two_runs_and_another_stream_give_equal_output(models, scene, result):
    assert same(run(models, scene), result)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = run(models, scene)
    side.synchronize()
    assert same(other, result)


def test_an_instance_alone_gives_its_rows_of_the_batch(models, scene, result):
    for n in (0, 4, 9, 39):
        alone = run(models, scene, sel=[n])
        for k in ('px_count_all', 'px_count_valid', 'px_count_visib', 'bbox_obj', 'bbox_visib', 'visib_fract', 'mask', 'mask_visib'):
            assert torch.equal(alone[k][0], result[k][n]), (n, k)
        assert int(alone['id_in_segm'][0]) == 1
        assert torch.equal(alone['mask_visib_all'][scene['view'][n]] > 0, result['mask_visib'][n])


def test_empty_batch(models, scene):
    out = run(models, scene, sel=[])
    assert out['px_count_all'].shape == (0,) and out['bbox_obj'].shape == (0, 4) and out['visib_fract'].shape == (0,) and out['mask'].shape == (0,) + HW
    assert out['mask_visib_all'].shape == (N_VIEWS,) + HW and not out['mask_visib_all'].any() and out['mask_visib_all'].is_cuda


def test_non_finite_pose_and_K_row_give_zeros_and_leave_the_others(models, scene, result):
    s = scene
    rows = ('px_count_all', 'px_count_valid', 'px_count_visib', 'bbox_obj', 'bbox_visib', 'visib_fract', 'mask', 'mask_visib')

    def check(out, bad):
        for n in range(len(s['obj'])):
            if bad[n]:
                assert not out['px_count_all'][n].any() and not out['px_count_valid'][n].any() and not out['px_count_visib'][n].any(), n
                assert (out['bbox_obj'][n] == -1).all() and (out['bbox_visib'][n] == -1).all() and out['visib_fract'][n] == 0, n
                assert not out['mask'][n].any() and not out['mask_visib'][n].any(), n
            else:
                for k in rows:
                    assert torch.equal(out[k][n], result[k][n]), (n, k)
        assert torch.equal(out['id_in_segm'], result['id_in_segm'])
        want_all = gr.composite_ref(np.stack([r['mask_visib'] & (not bad[n]) for n, r in enumerate(s['ref32'])]), s['view'], N_VIEWS)
        assert np.array_equal(out['mask_visib_all'].cpu().numpy(), want_all)

    T2 = s['TCO'].copy()
    T2[0, 0, 3] = np.nan; T2[12, 1, 1] = np.inf
    check(run(models, s, TCO=T2), np.isin(np.arange(len(s['obj'])), (0, 12)))
    K2 = s['K'].copy(); K2[2, 0, 0] = np.nan
    check(run(models, s, K=K2), s['view'] == 2)


def test_refusals_on_the_host(models, scene):
    from cosypose_amd import gt_info
    from cosypose_amd._lib import CosyHipError
    s = scene
    T, K, depth = dev(s['TCO'][:4]), dev(s['K']), dev(s['depth'])
    for o, v in (([0, 1, 3, 0], [0, 0, 0, 0]), ([0, -1, 2, 0], [0, 0, 0, 0]), ([0, 1, 2, 0], [0, 3, 0, 0]), ([0, 1, 2, 0], [0, -1, 0, 0])):
        with pytest.raises(ValueError, match='outside'):
            gt_info(T, o, v, K, depth, models)
    with pytest.raises(ValueError, match='holds 256 instances'):
        gt_info(dev(np.tile(s['TCO'][:1], (256, 1, 1))), [0] * 256, [1] * 256, K, depth, models)
    with pytest.raises(CosyHipError):
        gt_info(T.cpu(), [0, 1, 2, 0], [0, 0, 0, 0], K, depth, models)


def test_argument_checks_leave_the_outputs_untouched(models, scene):
    """bad arguments go through the C entry's checks only: a code comes back and nothing is launched"""
    from cosypose_amd._lib import lib, ptr
    l = lib()
    N = 4
    H, W = HW
    view, ids = dev(np.zeros(N, np.int32)), dev(np.arange(1, N + 1, dtype=np.int32))
    boxes, off = dev(np.tile(np.array([2 ** 31 - 1, 2 ** 31 - 1, -1, -1], np.int32), (N, 1))), dev(np.full(N, -1, np.int64))      # empty boxes: no window is read
    store, depth, K = torch.zeros(16, device='cuda'), dev(scene['depth']), dev(scene['K'])
    out = torch.full((N, 11), 7, dtype=torch.int32, device='cuda')
    comp = torch.full((N_VIEWS, H, W), 7, dtype=torch.int32, device='cuda')
    need = l.cosy_gt_info_workspace_bytes(N)
    ws = torch.zeros(need + 16, dtype=torch.uint8, device='cuda')
    counts, bo, bv = out[:, :3].contiguous(), out[:, 3:7].contiguous(), out[:, 7:].contiguous()
    args = lambda **kw: [kw.get(k, val) for k, val in dict(view=ptr(view), ids=ptr(ids), boxes=ptr(boxes), off=ptr(off), win=ptr(store), n_px=16, depth=ptr(depth),
                                                          K=ptr(K), delta=0.015, N=N, n_views=N_VIEWS, H=H, W=W, counts=ptr(counts), bo=ptr(bo), bv=ptr(bv),
                                                          comp=ptr(comp), mask=None, mv=None, ws=ptr(ws), wb=need, st=None).items()]
    for bad in (dict(N=-1), dict(n_views=0), dict(H=0), dict(n_px=-1), dict(view=None), dict(boxes=None), dict(win=None), dict(depth=None), dict(counts=None),
                dict(comp=None), dict(ws=None), dict(wb=need - 1), dict(ws=ptr(ws) + 4)):
        assert l.cosy_gt_info(*args(**bad)) == -1, bad
        torch.cuda.synchronize()
        assert (counts == 7).all() and (bo == 7).all() and (bv == 7).all() and (comp == 7).all(), bad
    assert l.cosy_gt_info(*args()) == 0
    torch.cuda.synchronize()
    assert (counts == 0).all() and (bo == -1).all() and (bv == -1).all() and (comp == 7).all()          # written in full; the composite only accumulates


# ---- (D) annotate_gt end to end -------------------------------------------------------------------------------------------------------------------
def test_annotate_gt_feeds_the_meters_and_the_valid_set_is_the_twins():
    from cosypose_amd import BopModels, BopScoreMeter, DetectionMeter, HipBatchRenderer, HipSceneRenderer, PandasTensorCollection, annotate_gt, synthetic as syn
    from cosypose_amd.io_formats import scene_gt_info_rows
    from cosypose_amd.pose_meters import prepare_candidates
    case = br.e2e_case()
    labels = case['labels']
    verts, faces, colors = syn.make_render_meshes(9, len(labels), 12, 16)
    e2e_models = BopModels(labels, verts, faces, colors_list=colors).cuda()
    H, W = br.E2E_HW
    meter, det = BopScoreMeter(e2e_models), DetectionMeter(visib_gt_min=0.1)
    scene_renderer, renderer = HipSceneRenderer(e2e_models.meshes), HipBatchRenderer(e2e_models.meshes)
    n_valid = n_gt = 0
    for scene_id, s in case['scenes'].items():
        names = np.asarray(labels)
        gt_infos = pd.DataFrame(dict(scene_id=s['gt']['scene_id'], view_id=s['gt']['view_id'], label=names[s['gt']['label']]))      # no visib_fract
        pred_infos = pd.DataFrame(dict(scene_id=s['pred']['scene_id'], view_id=s['pred']['view_id'], label=names[s['pred']['label']], score=s['pred']['score']))
        cameras = PandasTensorCollection(pd.DataFrame(dict(scene_id=s['cameras']['scene_id'], view_id=s['cameras']['view_id'])), K=dev(s['cameras']['K']))
        K = s['cameras']['K']
        # the measured depth: the scene's own render, and a wall 30 cm from the camera over the left 45 % of the frame
        depth = scene_renderer.render(gt_infos['label'].values, s['gt']['view_id'], dev(s['gt']['poses']), dev(K), (H, W), render_depth=True)['depth'].clone()
        depth[:, :, :int(0.45 * W)] = 0.3
        annotated, mask_all = annotate_gt(PandasTensorCollection(gt_infos, poses=dev(s['gt']['poses'])), cameras, depth, e2e_models)
        torch.cuda.synchronize()
        # the twin on the package's canvas renders
        view = s['gt']['view_id'].astype(np.int64)                                      # cameras are in view order
        Kc = K.copy(); Kc[:, 0, 2] = Kc[:, 0, 2] + np.float32(W); Kc[:, 1, 2] = Kc[:, 1, 2] + np.float32(H)
        _, D_large = renderer.render([dict(name=l) for l in gt_infos['label']], dev(s['gt']['poses']), dev(Kc[view]), resolution=(3 * H, 3 * W), render_depth=True)
        D_large, depth_h = D_large.cpu().numpy(), depth.cpu().numpy()
        ref = [gr.gt_info_ref(D_large[n], depth_h[view[n]], K[view[n]]) for n in range(len(view))]
        fract = np.array([r['visib_fract'] for r in ref])
        print('scene', scene_id, 'visib_fract', np.round(fract, 4).tolist())
        assert np.array_equal(annotated.infos['visib_fract'].values, fract)
        for k in ('px_count_all', 'px_count_valid', 'px_count_visib'):
            assert np.array_equal(annotated.infos[k].values, [r[k] for r in ref]), k
        assert np.array_equal(annotated.infos['id_in_segm'].values, gr.id_in_segm_ref(view))
        assert np.array_equal(annotated.bbox_visib.cpu().numpy(), [r['bbox_visib'] for r in ref]) and np.array_equal(annotated.bbox_obj.cpu().numpy(), [r['bbox_obj'] for r in ref])
        bv = annotated.bbox_visib.cpu().numpy().astype(np.float32)
        assert annotated.bboxes.dtype == torch.float32 and np.array_equal(annotated.bboxes.cpu().numpy(), np.stack([bv[:, 0], bv[:, 1], bv[:, 0] + bv[:, 2], bv[:, 1] + bv[:, 3]], 1))
        assert np.array_equal(mask_all.cpu().numpy(), gr.composite_ref(np.stack([r['mask_visib'] for r in ref]), view, len(K)))
        assert torch.equal(annotated.poses, dev(s['gt']['poses']))
        rows = scene_gt_info_rows(annotated)
        assert sum(len(v) for v in rows.values()) == len(view) and set(rows) == {(scene_id, int(v)) for v in view}
        # straight into the meters: the valid ground truth is what the twin's fractions give
        preds = PandasTensorCollection(pred_infos, poses=dev(s['pred']['poses']), bboxes=torch.zeros(len(pred_infos), 4, device='cuda'))
        meter.add(preds, annotated, cameras, depth)
        det.add(preds, annotated)
        valid = prepare_candidates(pred_infos, annotated.infos, visib_gt_min=0.1)['gt_infos']['valid'].values.astype(bool)
        assert np.array_equal(valid, fract >= 0.1)
        assert np.abs(fract - 0.1).min() > 0.01                                          # no fraction sits at the threshold
        n_valid += int((fract >= 0.1).sum()); n_gt += len(fract)
    summary, _ = meter.summary()
    print('valid ground truth', n_valid, 'of', n_gt)
    assert summary['n_gt_valid'] == n_valid and summary['n_gt'] == n_gt and 0 < n_valid < n_gt
