"""CPU tests of the BOP ground-truth annotations: the numpy twin (tests/gt_ref.py) against hand values, the host half of
cosypose_amd/gt_annotations.py (chunks, id_in_segm, refusals, box conventions), io_formats.scene_gt_info_rows, and the C ABI's host-side
argument checks.  No GPU."""
import pathlib

import numpy as np
import pandas as pd
import pytest
import torch

import bop_ref as br
import gt_ref as gr

REPO = pathlib.Path(__file__).resolve().parent.parent
KEYS = ('px_count_all', 'px_count_valid', 'px_count_visib', 'visib_fract', 'bbox_obj', 'bbox_visib')


# ---- the twin against hand values (no package code) ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', gr.hand_cases(), ids=lambda c: c[0])
def test_hand_values(case):
    name, D_large, D_test, want = case
    got32, got64 = gr.gt_info_ref(D_large, D_test, br.HAND_K), gr.gt_info_ref(D_large, D_test, br.HAND_K, exact=True)
    print(name, {k: got32[k] for k in KEYS})
    for k, v in want.items():
        assert got32[k] == v and got64[k] == v, (k, got32[k], got64[k], v)
    # no pixel of a hand case is near the threshold: float32 and float64 decide alike
    assert not got64['undecided'].any() and np.array_equal(got32['mask_visib'], got64['mask_visib']) and np.array_equal(got32['mask'], got64['mask'])


def test_hand_case_properties_named_by_the_contract():
    cases = {c[0]: gr.gt_info_ref(c[1], c[2], br.HAND_K) for c in gr.hand_cases()}
    a = cases['fully inside, sensor equal']
    assert a['px_count_all'] == a['px_count_valid'] == a['px_count_visib'] and a['visib_fract'] == 1.0
    assert cases['sensor 1 cm nearer']['visib_fract'] == 1.0
    h = cases['sensor 2 cm nearer']
    assert h['visib_fract'] == 0.0 and h['bbox_obj'] == [-1] * 4 and h['bbox_visib'] == [-1] * 4 and h['px_count_all'] == 256
    m = cases['sensor missing on half']
    assert m['visib_fract'] == 1.0 and m['px_count_valid'] * 2 == m['px_count_all']
    o = cases['occluder 10 cm in front of half']
    assert o['visib_fract'] == 0.5 and o['bbox_visib'] == [16, 16, 7, 15] and o['mask_visib'][16:32, 16:24].all() and not o['mask_visib'][:, 24:].any()
    l = cases['half left of the frame']
    assert l['px_count_all'] == 256 and l['visib_fract'] <= 0.5 and l['bbox_obj'][0] < 0 and l['mask'].sum() == 128
    out = cases['outside the frame, on the canvas']
    assert out['px_count_all'] > 0 and out['px_count_valid'] == out['px_count_visib'] == 0 and out['visib_fract'] == 0.0 and not out['mask'].any()
    n = cases['one NaN sensor pixel']
    assert n['mask'][20, 20] and not n['mask_visib'][20, 20] and n['px_count_valid'] == 255 and n['px_count_visib'] == 255


def test_composite_holds_the_higher_id_where_two_visible_masks_overlap():
    D_large, D_test = gr.overlap_case()
    a, b = (gr.gt_info_ref(D_large[n], D_test, br.HAND_K) for n in (0, 1))
    both = a['mask_visib'] & b['mask_visib']
    assert both.sum() == 16 * 8 and a['visib_fract'] == 1.0 and b['visib_fract'] == 1.0         # 1 cm apart: both visible where they overlap
    comp = gr.composite_ref(np.stack([a['mask_visib'], b['mask_visib']]), [0, 0], 1)
    assert comp.dtype == np.uint8 and (comp[0][both] == 2).all() and (comp[0][a['mask_visib'] & ~both] == 1).all() and (comp[0][b['mask_visib']] == 2).all()
    assert (comp[0][~(a['mask_visib'] | b['mask_visib'])] == 0).all()
    # rows of another view in between do not change the ids of this one
    comp3 = gr.composite_ref(np.stack([a['mask_visib'], b['mask_visib'], b['mask_visib']]), [0, 1, 0], 2)
    assert np.array_equal(comp3[0], comp[0]) and (comp3[1][b['mask_visib']] == 1).all()


def test_an_undecided_pixel_is_marked_and_only_there_may_the_twins_differ():
    sq = gr.canvas_square(1.0, 16, 32)
    dg = br.dist64(gr.crop(sq), br.HAND_K)
    D_test = gr.crop(sq)
    # the sensor such that dist_gt - t at pixel (20, 20) is delta up to the rounding of the sensor value itself
    scale = dg[20, 20] / 1.0
    D_test[20, 20] = np.float32((dg[20, 20] - float(np.float32(gr.DELTA))) / scale)
    r64 = gr.gt_info_ref(sq, D_test, br.HAND_K, exact=True)
    r32 = gr.gt_info_ref(sq, D_test, br.HAND_K)
    # the rounding of the sensor value (0.5 u) lies inside 13 u: the pixel is undecided
    assert r64['undecided'][20, 20] and r64['undecided'].sum() == 1
    assert np.array_equal(r32['mask_visib'][~r64['undecided']], r64['mask_visib'][~r64['undecided']])


# ---- the host half of gt_annotations ----------------------------------------------------------------------------------------------------------
def test_chunks_hold_every_instance_once_and_stay_under_the_cap():
    from cosypose_amd.gt_annotations import plan_chunks
    rs = np.random.RandomState(0)
    x0, y0 = rs.randint(0, 100, 40), rs.randint(0, 100, 40)
    boxes = np.stack([x0, y0, x0 + rs.randint(0, 60, 40), y0 + rs.randint(0, 60, 40)], 1)
    boxes[3] = [5, 5, 4, 9]; boxes[4] = [2 ** 31 - 1, 2 ** 31 - 1, -1, -1]; boxes[17] = [2 ** 31 - 1, 2 ** 31 - 1, -2, -2]      # empty and dead boxes
    size = np.maximum(boxes[:, 2] - boxes[:, 0] + 1, 0) * np.maximum(boxes[:, 3] - boxes[:, 1] + 1, 0)
    assert size[3] == size[4] == size[17] == 0
    one = plan_chunks(boxes)
    assert len(one) == 1 and (one[0]['lo'], one[0]['hi']) == (0, 40) and one[0]['n_pixels'] == size.sum()
    assert plan_chunks(np.zeros((0, 4), int)) == []
    for cap in (int(size.max()), int(size.max()) * 2, int(size.sum()) - 1, int(size.sum())):
        chunks = plan_chunks(boxes, cap)
        assert chunks[0]['lo'] == 0 and chunks[-1]['hi'] == 40 and all(a['hi'] == b['lo'] for a, b in zip(chunks, chunks[1:]))
        assert all(c['hi'] > c['lo'] for c in chunks)
        for c in chunks:
            s, off = size[c['lo']:c['hi']], c['win_offset']
            assert c['n_pixels'] == s.sum() <= cap and off.dtype == np.int64 and len(off) == len(s)
            assert np.array_equal(off[s == 0], np.full((s == 0).sum(), -1))
            assert np.array_equal(off[s > 0], (np.cumsum(s) - s)[s > 0])          # packed, in order, no overlap
        assert (len(chunks) == 1) == (cap >= size.sum())
    assert len(plan_chunks(boxes, int(size.max()))) >= 3
    with pytest.raises(ValueError, match=rf'instance {int(np.argmax(size))} alone needs {int(size.max())} \({4 * int(size.max())} bytes\)'):
        plan_chunks(boxes, int(size.max()) - 1)


def test_id_in_segm_ranks_rows_within_their_view():
    from cosypose_amd.gt_annotations import id_in_segm_of
    view = [2, 0, 2, 1, 0, 2, 2]
    got = id_in_segm_of(view)
    assert got.dtype == np.int32 and got.tolist() == [1, 1, 2, 1, 2, 3, 4] and np.array_equal(got, gr.id_in_segm_ref(view))
    assert id_in_segm_of([]).shape == (0,)
    assert id_in_segm_of([0] * 255 + [1]).max() == 255
    with pytest.raises(ValueError, match='view 3 holds 256 instances'):
        id_in_segm_of([3, 1] * 256)


def cpu_models():
    from cosypose_amd import BopModels
    v = np.array([[-0.04, -0.04, 0], [0.04, -0.04, 0], [0.04, 0.04, 0], [-0.04, 0.04, 0]], np.float32)
    return BopModels(['obj_000001'], [v], [np.array([[0, 1, 2], [0, 2, 3]], np.int32)])


def test_cpu_tensors_are_refused():
    from cosypose_amd import gt_info
    from cosypose_amd._lib import CosyHipError
    T = torch.eye(4)[None]
    with pytest.raises(CosyHipError, match='no CPU fallback'):
        gt_info(T, [0], [0], torch.from_numpy(br.HAND_K)[None], torch.ones(1, 48, 64), cpu_models())


def test_lazy_exports():
    import cosypose_amd
    from cosypose_amd import gt_info, annotate_gt
    assert gt_info.__module__ == 'cosypose_amd.gt_annotations' and annotate_gt is cosypose_amd.gt_annotations.annotate_gt


def test_xywh_to_xyxy_and_the_canvas_intrinsics():
    from cosypose_amd.gt_annotations import xywh_to_xyxy, canvas_K
    got = xywh_to_xyxy(torch.tensor([[3, 4, 10, 0], [-1, -1, -1, -1], [0, 7, 63, 40]], dtype=torch.int32))
    assert got.dtype == torch.float32 and got.tolist() == [[3, 4, 13, 4], [-1, -1, -2, -2], [0, 7, 63, 47]]
    K = torch.from_numpy(br.make_K(2, 48, 64)); K[1, 0, 2] = 0.1
    Kc = canvas_K(K, (48, 64))
    want = K.numpy().copy(); want[:, 0, 2] = want[:, 0, 2] + np.float32(64); want[:, 1, 2] = want[:, 1, 2] + np.float32(48)
    assert np.array_equal(Kc.numpy(), want) and Kc.dtype == torch.float32 and K[1, 0, 2] == np.float32(0.1)      # one float32 addition, K untouched


def test_scene_gt_info_rows_types_and_keys():
    from cosypose_amd import PandasTensorCollection
    from cosypose_amd.io_formats import scene_gt_info_rows
    infos = pd.DataFrame(dict(scene_id=[4, 4, 9], view_id=[1, 0, 1], label=['a', 'b', 'a'], visib_fract=[0.5, 0.0, 1.0],
                              px_count_all=np.array([10, 7, 3]), px_count_valid=np.array([9, 0, 3]), px_count_visib=np.array([5, 0, 3]), id_in_segm=[1, 1, 1]))
    ann = PandasTensorCollection(infos, poses=torch.eye(4).repeat(3, 1, 1),
                                 bbox_obj=torch.tensor([[-3, 2, 8, 9], [-1, -1, -1, -1], [1, 1, 1, 2]], dtype=torch.int32),
                                 bbox_visib=torch.tensor([[0, 2, 5, 9], [-1, -1, -1, -1], [1, 1, 1, 2]], dtype=torch.int32))
    rows = scene_gt_info_rows(ann)
    assert list(rows) == [(4, 1), (4, 0), (9, 1)] and all(len(v) == 1 for v in rows.values())
    r = rows[(4, 1)][0]
    assert set(r) == {'bbox_obj', 'bbox_visib', 'px_count_all', 'px_count_valid', 'px_count_visib', 'visib_fract'}
    assert r == dict(bbox_obj=[-3, 2, 8, 9], bbox_visib=[0, 2, 5, 9], px_count_all=10, px_count_valid=9, px_count_visib=5, visib_fract=0.5)
    for row in (v[0] for v in rows.values()):
        assert all(type(x) is int for k in ('bbox_obj', 'bbox_visib') for x in row[k]) and type(row['visib_fract']) is float
        assert all(type(row[k]) is int for k in ('px_count_all', 'px_count_valid', 'px_count_visib'))
    import json
    json.dumps({f'{k[1]}': v for k, v in rows.items()})                      # plain values: serialisable as they are
    two = scene_gt_info_rows(PandasTensorCollection(pd.concat([infos, infos.iloc[:1]]), poses=torch.eye(4).repeat(4, 1, 1),
                                                    bbox_obj=ann.bbox_obj[[0, 1, 2, 0]], bbox_visib=ann.bbox_visib[[0, 1, 2, 0]]))
    assert len(two[(4, 1)]) == 2                                               # rows of one image stay in annotation order


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------------
GT_SYMBOLS = ('cosy_gt_info_workspace_bytes', 'cosy_gt_info', 'cosy_gt_composite_u8')


def test_c_abi_declares_exports_and_builds_the_gt_entry_points():
    from cosypose_amd import _lib
    from cosypose_amd.build import build, SOURCES, FILE_FLAGS
    build()
    for name in GT_SYMBOLS:
        assert name in _lib.EXPORTS, name           # test_c_abi.py: EXPORTS, the header and the built library name the same entry points
    assert 'kernels_gt.hip' in SOURCES and '-ffp-contract=off' in FILE_FLAGS['kernels_gt.hip']
    # both files compile one text of the distance function and the window helpers
    bop, gt = ((REPO / 'cosypose_amd' / 'csrc' / f).read_text() for f in ('kernels_bop.hip', 'kernels_gt.hip'))
    assert '#include "bop_device.h"' in bop and '#include "bop_device.h"' in gt and 'float depth_to_dist(' not in bop and 'float depth_to_dist(' not in gt


def test_argument_checks_run_on_the_host_before_any_launch():
    """COSY_EINVAL (-1) with the argument named, and N = 0 returns COSY_OK with null pointers: neither touches a device"""
    from cosypose_amd._lib import lib
    l = lib()
    P = 64          # a non-null, 16-byte aligned stand-in: every call below is refused (or returns) before a pointer is used
    assert l.cosy_gt_info_workspace_bytes(0) == 0 and l.cosy_gt_info_workspace_bytes(-3) == 0
    need = l.cosy_gt_info_workspace_bytes(7)
    assert need % 16 == 0 and need >= 8 + 8 * 4 + 7 * 11 * 4

    def info(**kw):
        a = dict(view=P, ids=P, boxes=P, off=P, win=P, n_px=100, depth=P, K=P, delta=0.015, N=7, n_views=2, H=48, W=64, counts=P, bo=P, bv=P, comp=P,
                 mask=None, mv=None, ws=P, wb=need, st=None)
        a.update(kw)
        return l.cosy_gt_info(*a.values())
    for bad, word in ((dict(N=-1), b'N=-1'), (dict(n_views=0), b'n_views=0'), (dict(H=0), b'H=0'), (dict(W=-2), b'W=-2'), (dict(n_px=-1), b'n_pixels=-1'),
                      (dict(view=None), b'null inst_view'), (dict(ids=None), b'null id_in_segm'), (dict(boxes=None), b'null boxes'),
                      (dict(off=None), b'null win_offset'), (dict(win=None), b'null windows'), (dict(depth=None), b'null depth_test'),
                      (dict(K=None), b'null K'), (dict(counts=None), b'null counts'), (dict(bo=None), b'null bbox_obj'), (dict(bv=None), b'null bbox_visib'),
                      (dict(comp=None), b'null composite'), (dict(ws=None), b'null workspace'), (dict(wb=need - 1), b'workspace_bytes='),
                      (dict(ws=P + 4), b'16-byte'), (dict(H=20000, W=20000), b'canvas'), (dict(N=1 << 30, H=480, W=640), b'2^31 items')):
        assert info(**bad) == -1 and word in l.cosy_last_error(), (bad, l.cosy_last_error())
    assert info(N=0, view=None, ids=None, boxes=None, off=None, win=None, depth=None, K=None, counts=None, bo=None, bv=None, comp=None, ws=None, wb=0) == 0
    assert l.cosy_gt_composite_u8(None, 0, None, None) == 0
    for args, word in (((P, -1, P, None), b'n=-1'), ((None, 5, P, None), b'null composite'), ((P, 5, None, None), b'null out')):
        assert l.cosy_gt_composite_u8(*args) == -1 and word in l.cosy_last_error(), (args, l.cosy_last_error())
