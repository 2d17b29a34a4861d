"""CPU tests of the host side: the C ABI exports what include/cosyhip.h declares (no compute
calls without a GPU), containers, mesh DB, sharding, state-dict layout, factories."""
import argparse
import ctypes
import os
import re
import pathlib

import numpy as np
import pandas as pd
import pytest
import torch

REPO = pathlib.Path(__file__).resolve().parent.parent


def test_c_abi_exports_every_declared_symbol():
    from cosypose_amd.build import build, LIB
    build()  # hipcc cross-compiles for gfx950 without a GPU
    header = (REPO / 'include' / 'cosyhip.h').read_text()
    code = re.sub(r'/\*.*?\*/', '', header, flags=re.S)          # prototypes only, comments stripped
    declared = set(re.findall(r'\b(cosy_[a-z0-9_]+)\s*\(', code))
    assert len(declared) >= 18
    lib = ctypes.CDLL(LIB)
    for name in sorted(declared):
        assert hasattr(lib, name), f'{name} declared in cosyhip.h but not exported'
    from cosypose_amd import _lib
    assert set(_lib.EXPORTS) == declared, set(_lib.EXPORTS) ^ declared
    l = _lib.lib()
    assert l.cosy_version() == 100
    assert l.cosy_effnet_b3_param_count() == 10798441
    oh, ow = ctypes.c_int(), ctypes.c_int()
    assert l.cosy_effnet_b3_out_hw(240, 320, ctypes.byref(oh), ctypes.byref(ow)) == 0
    assert (oh.value, ow.value) == (7, 10)          # the static-padding quirk (15x20 -> 7x10)
    # error path without a GPU: a wrong blob size is rejected before any device work
    blob = np.zeros(10, np.float32)
    h = ctypes.c_void_p()
    rc = l.cosy_effnet_b3_create(blob.ctypes.data, 10, 1, 240, 320, 4, ctypes.byref(h))
    assert rc == -4 and b'10798441' in l.cosy_last_error()


def test_product_never_imports_the_oracle():
    for f in list((REPO / 'cosypose_amd').rglob('*.py')):
        code = [l for l in f.read_text().splitlines() if 'import' in l or 'sys.path' in l or 'CDLL' in l]
        assert not any('oracle' in l for l in code), f


def test_cpu_tensors_are_rejected():
    from cosypose_amd import lib3d
    from cosypose_amd._lib import CosyHipError
    with pytest.raises(CosyHipError):
        lib3d.update_pose(torch.eye(4)[None], torch.eye(3)[None], torch.ones(1, 9))


def test_state_dict_layout_and_factories(golden, golden_sd, oracle):
    from cosypose_amd.pose_models_cfg import create_model_pose, create_model_coarse, create_model_refiner, check_update_config
    from cosypose_amd.efficientnet import flat_params
    cfg = check_update_config(argparse.Namespace(backbone_str='efficientnet-b3', n_pose_dims=9))
    assert cfg.init_method == 'v0'
    m = create_model_pose(cfg, renderer=None, mesh_db=None)
    assert m.render_size == (240, 320) and m.pose_dim == 9 and m.backbone.n_features == 1536 and m.backbone.n_inputs == 6
    assert set(m.heads) == {'pose'} and m.heads['pose'] is m.pose_fc and m.debug is False
    # reference checkpoints load unchanged: same keys (incl. num_batches_tracked) and shapes
    ref_keys, ref_shapes = list(golden['sd_keys']), golden['sd_shapes']
    sd = m.state_dict()
    assert list(sd.keys()) == ref_keys
    for k, shp in zip(ref_keys, ref_shapes):
        assert tuple(sd[k].shape) == tuple(int(v) for v in shp if v >= 0), k
    full = {k: torch.from_numpy(v) for k, v in golden_sd.items()}
    full.update({k: torch.tensor(0) for k in ref_keys if k.endswith('num_batches_tracked')})
    m.load_state_dict(full, strict=True)
    blob, _ = flat_params(m.backbone, m.pose_fc)
    assert np.array_equal(blob.numpy(), oracle.flatten_state_dict(golden_sd))
    for bad in ('flownet', 'resnet34', 'vgg'):
        with pytest.raises(ValueError):
            create_model_coarse(argparse.Namespace(backbone_str=bad, n_pose_dims=9), None, None)
    assert type(create_model_refiner(cfg, None, None)) is type(m)


def test_tensor_collections():
    from cosypose_amd import tensor_collection as tc
    infos = pd.DataFrame(dict(label=['a', 'b', 'c'], batch_im_id=[0, 0, 1], score=[.9, .8, .7]))
    c = tc.PandasTensorCollection(infos, poses=torch.arange(48.).reshape(3, 4, 4), bboxes=torch.zeros(3, 4))
    assert len(c) == 3 and c.poses.shape == (3, 4, 4) and set(c.tensors) == {'poses', 'bboxes'}
    sub = c[[2, 0]]
    assert list(sub.infos['label']) == ['c', 'a'] and torch.equal(sub.poses, c.poses[[2, 0]])
    cat = tc.concatenate([c[[0]], c[[]], c[[1, 2]]])
    assert list(cat.infos['label']) == ['a', 'b', 'c'] and torch.equal(cat.poses, c.poses)
    assert len(tc.concatenate([c[[]]])) == 0
    # a single non-empty part is handed on as it is (fresh index, same tensors: no row copies), empty parts beside it are dropped
    one = tc.concatenate([c[[]], c[[1, 2]], c[[]]])
    assert list(one.infos['label']) == ['b', 'c'] and list(one.infos.index) == [0, 1] and torch.equal(one.poses, c.poses[1:])
    assert set(one.tensors) == {'poses', 'bboxes'}
    c.register_tensor('K_crop', torch.ones(3, 3, 3))
    import pickle
    c2 = pickle.loads(pickle.dumps(c))
    assert list(c2.infos['label']) == ['a', 'b', 'c'] and torch.equal(c2.K_crop, c.K_crop)
    with pytest.raises(AttributeError):
        c.nope
    assert c.float().poses.dtype == torch.float32 and c.clone().poses is not c.poses


def test_mesh_db_matches_reference_sampling(golden):
    from cosypose_amd.mesh_db import BatchedMeshes
    from cosypose_amd import synthetic as syn
    labels = np.array([f'o{i}' for i in range(4)])
    pts = torch.from_numpy(syn.make_mesh_points(7, 4, 2500))
    db = BatchedMeshes({l: dict(label=l, n_sym=1) for l in labels}, labels, pts, torch.eye(4).reshape(1, 1, 4, 4).repeat(4, 1, 1, 1))
    sel = db.select(['o2', 'o0']).sample_points(2000, deterministic=True)
    ids = golden['sample_ids_2500']  # what the reference's sample_points(2000, deterministic=True) drew
    assert torch.equal(sel, pts[[2, 0]][:, ids])
    assert torch.equal(db.point_table(2000), pts[:, ids])
    assert db.object_ids(['o3', 'o1']).tolist() == [3, 1]
    assert db.n_sym_mapping == {l: 1 for l in labels}


def test_sharding():
    from cosypose_amd.distributed import shard_range, balanced_assignment
    for n in (0, 1, 7, 1024, 2048, 1001):
        for world in (1, 2, 8):
            spans = [shard_range(n, r, world) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
            assert [e - s for s, e in spans] == [len(x) for x in np.array_split(np.arange(n), world)]
    costs = np.array([4] * 10 + [1] * 40, float)
    parts = balanced_assignment(costs, 8)
    loads = [costs[p].sum() for p in parts]
    assert sorted(np.concatenate(parts).tolist()) == list(range(50)) and max(loads) - min(loads) <= 4


def test_detection_and_bop_csv_formats(tmp_path):
    """detector output contract (detector.py:19-72) and the BOP csv round trip (run_custom_scenario.py:26-58)"""
    import pandas as pd
    from cosypose_amd import io_formats, tensor_collection as tc
    from cosypose_amd import synthetic as syn
    per_image = [dict(boxes=np.array([[10, 20, 110, 220], [5, 5, 50, 60], [30, 40, 90, 100]], np.float32),
                      labels=np.array(['obj_000002', 'obj_000005', 'obj_000002']), scores=np.array([0.9, 0.2, 0.95])),
                 dict(boxes=np.zeros((0, 4), np.float32), labels=np.array([]), scores=np.array([])),
                 dict(boxes=np.array([[1, 2, 3, 4]], np.float32), labels=np.array(['obj_000007']), scores=np.array([0.5]))]
    det = io_formats.make_detections(per_image, device='cpu')
    assert list(det.infos.columns) == ['batch_im_id', 'label', 'score'] and det.bboxes.shape == (4, 4)
    assert det.infos['batch_im_id'].tolist() == [0, 0, 0, 2]
    det = io_formats.make_detections(per_image, device='cpu', detection_th=0.3)
    assert det.infos['label'].tolist() == ['obj_000002', 'obj_000002', 'obj_000007']
    det = io_formats.make_detections(per_image, device='cpu', detection_th=0.3, one_instance_per_class=True)
    assert sorted(zip(det.infos['label'], det.infos['score'])) == [('obj_000002', 0.95), ('obj_000007', 0.5)]
    assert det.bboxes[det.infos['label'].tolist().index('obj_000002')].tolist() == [30, 40, 90, 100]
    assert len(io_formats.make_detections([dict(boxes=np.zeros((0, 4)), labels=[], scores=[])], device='cpu')) == 0
    # refined poses -> BOP csv (t in mm, row-major R) -> candidates
    poses = torch.from_numpy(syn.make_TCO(5, 3))
    infos = pd.DataFrame(dict(label=['obj_000002', 'obj_000007', 'obj_000021'], score=[0.9, 0.5, 0.25], scene_id=[48, 48, 49], view_id=[1, 1, 733]))
    preds = tc.PandasTensorCollection(infos=infos, poses=poses)
    path = tmp_path / 'bop.csv'
    io_formats.tc_to_csv(preds, path)
    lines = path.read_text().split('\n')
    assert lines[0] == 'scene_id,im_id,obj_id,score,R,t,time' and len(lines) == 4
    f = lines[1].split(',')
    assert f[:3] == ['48', '1', '2'] and len(f[4].split(' ')) == 9 and len(f[5].split(' ')) == 3
    assert abs(float(f[5].split(' ')[2]) - 1e3 * float(poses[0, 2, 3])) < 1e-3        # millimetres
    back = io_formats.read_csv_candidates(path)
    assert back.infos['label'].tolist() == infos['label'].tolist() and back.infos['view_id'].tolist() == [1, 1, 733]
    assert torch.allclose(back.poses, poses, atol=1e-6)


def test_io_formats_vs_reference_fixtures(tmp_path):
    """io_formats against what the reference's own Detector.get_detections (detector.py:36-72) and run_custom_scenario
    (:26-58) produced on the same inputs (tests/golden/generate_golden_io.py): every option of the detector
    post-processing incl. the empty case, the csv reader on a literal BOP19 file, and the rows handed to the BOP writer."""
    import pandas as pd
    from conftest import REPO
    from cosypose_amd import io_formats, tensor_collection as tc
    g = dict(np.load(REPO / 'tests' / 'golden' / 'reference_golden_io.npz', allow_pickle=False))
    names = {int(i): str(n) for n, i in zip(g['det_label_names'], g['det_label_ids'])}
    per_image = [dict(boxes=g[f'det_in{i}_boxes'], labels=[names[int(c)] for c in g[f'det_in{i}_labels']], scores=g[f'det_in{i}_scores'],
                      masks=g[f'det_in{i}_masks']) for i in range(3)]
    cases = dict(plain={}, th=dict(detection_th=0.5), one=dict(one_instance_per_class=True),
                 masks=dict(output_masks=True, mask_th=0.6, detection_th=0.3), th_one=dict(detection_th=0.2, one_instance_per_class=True))
    for name, kw in cases.items():
        det = io_formats.make_detections(per_image, device='cpu', **kw)
        assert list(det.infos.columns) == list(g[f'det_{name}_columns']), name
        assert det.infos['batch_im_id'].tolist() == g[f'det_{name}_info_batch_im_id'].tolist(), name
        assert det.infos['label'].tolist() == g[f'det_{name}_info_label'].tolist(), name
        assert np.allclose(det.infos['score'].values, g[f'det_{name}_info_score'], rtol=0, atol=1e-7), name
        assert det.bboxes.dtype == torch.float32 and np.array_equal(det.bboxes.numpy(), g[f'det_{name}_bboxes']), name
        if f'det_{name}_masks' in g:
            assert det.masks.dtype == torch.bool and np.array_equal(det.masks.numpy(), g[f'det_{name}_masks'])
        else:
            assert 'masks' not in det.tensors
    empty = io_formats.make_detections([dict(boxes=np.zeros((0, 4)), labels=[], scores=[], masks=np.zeros((0, 1, 6, 8)))] * 3, device='cpu',
                                       output_masks=True)
    assert len(empty) == int(g['det_empty_n']) == 0 and list(empty.infos.columns) == list(g['det_empty_columns'])
    assert tuple(empty.bboxes.shape) == tuple(g['det_empty_bboxes_shape'])
    # csv reader on the literal file the reference read
    p = tmp_path / 'ref.csv'; p.write_text(str(g['csv_text']))
    cand = io_formats.read_csv_candidates(p)
    assert list(cand.infos.columns) == list(g['csv_columns'])
    for c in cand.infos.columns:
        want = g[f'csv_info_{c}']
        assert cand.infos[c].tolist() == want.tolist() if c == 'label' else np.allclose(cand.infos[c].values.astype(float), want.astype(float))
    assert cand.poses.dtype == torch.float32 and np.array_equal(cand.poses.numpy(), g['csv_poses'])
    # the rows the reference hands to the BOP writer; then our file read back by our reader
    infos = pd.DataFrame(dict(label=['obj_000005', 'obj_000021', 'obj_000001'], score=[0.87, 0.5, 0.125], scene_id=[48, 48, 7], view_id=[1, 1, 103]))
    preds = tc.PandasTensorCollection(infos=infos, poses=cand.poses.clone())
    rows = io_formats.bop19_rows(preds)
    assert sorted(rows[0]) == list(g['rows_keys'])
    for k in ('scene_id', 'im_id', 'obj_id', 'score', 'time'):
        assert np.allclose([float(r[k]) for r in rows], g[f'rows_{k}'])
    assert np.allclose(np.stack([r['t'] for r in rows]), g['rows_t'], rtol=0, atol=1e-9 * 1e3)
    assert np.allclose(np.stack([r['R'] for r in rows]), g['rows_R'], rtol=0, atol=0)
    out = tmp_path / 'ours.csv'
    io_formats.tc_to_csv(preds, out)
    assert out.read_text().split('\n')[0] == 'scene_id,im_id,obj_id,score,R,t,time'
    back = io_formats.read_csv_candidates(out)
    assert back.infos['label'].tolist() == infos['label'].tolist() and torch.allclose(back.poses, cand.poses, atol=1e-6)


def test_lr_schedule_matches_the_reference_scheduler_sequence():
    """training.LRSchedule (faithful mode) against torch's LambdaLR + StepLR driven exactly in the order of the reference
    (cosypose/training/train_pose.py:284-299 construction incl. the resume fast-forward, :331-334 stepping), fresh and resumed,
    with and without warm-up; and the `faithful=False` schedule continues across a resume."""
    import warnings
    from cosypose_amd.training import LRSchedule

    def reference_sequence(lr, n_warm, bpe, decay, start_epoch, end_epoch):
        p = torch.nn.Parameter(torch.zeros(1))
        opt = torch.optim.Adam([p], lr=lr)
        nbw = n_warm * bpe
        lambd = (lambda e: 1) if n_warm == 0 else (lambda b: (b + 1) / nbw)
        warm = torch.optim.lr_scheduler.LambdaLR(opt, lambd)
        warm.last_epoch = start_epoch * bpe
        sch = torch.optim.lr_scheduler.StepLR(opt, step_size=decay, gamma=0.1)
        sch.last_epoch = start_epoch - 1
        sch.step()
        out = []
        for e in range(start_epoch, end_epoch):
            for _ in range(bpe):
                out.append(opt.param_groups[0]['lr'])
                opt.step()
                if e < n_warm:
                    warm.step()
            if e >= n_warm:
                sch.step()
        return out
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for lr, n_warm, bpe, decay, start, end in [(1e-3, 2, 3, 2, 0, 8), (1e-3, 2, 3, 2, 3, 8), (1e-3, 0, 3, 2, 0, 6), (1e-3, 0, 3, 2, 4, 7),
                                                   (3e-4, 2, 3, 2, 1, 5), (3e-4, 50, 4, 100, 0, 60), (3e-4, 50, 4, 100, 55, 60)]:
            want = reference_sequence(lr, n_warm, bpe, decay, start, end)
            sch = LRSchedule(lr, n_warm, bpe, decay, start_epoch=start)
            got = []
            for e in range(start, end):
                for b in range(bpe):
                    got.append(sch.current(e, b)); sch.after_batch(e)
                sch.after_epoch(e)
            assert np.allclose(got, want, rtol=1e-12, atol=0), (lr, n_warm, bpe, decay, start)
    fresh = LRSchedule(1e-3, 2, 3, 2, faithful=False)
    resumed = LRSchedule(1e-3, 2, 3, 2, start_epoch=5, faithful=False)
    assert [fresh.current(e, b) for e in range(5, 8) for b in range(3)] == [resumed.current(e, b) for e in range(5, 8) for b in range(3)]
    assert abs(fresh.current(1, 2) - 1e-3) < 1e-15 and abs(fresh.current(4, 0) - 1e-3 * 7 / 6 * 0.1) < 1e-15


def test_add_noise_vs_reference_fixture():
    """h_pose's pose-noise generators ('gt+noise', 'fixed+trans_noise'): cosypose_amd.pose_forward_loss.add_noise against the
    outputs of the reference's own add_noise (cosypose/lib3d/transform_ops.py:35-51; tests/golden/generate_golden_noise.py binds
    scipy's static-axes Euler rotation in place of the absent transforms3d), same numpy seed: same poses, and the same
    number of RNG draws consumed."""
    import numpy as np
    import torch
    from conftest import REPO
    from cosypose_amd import synthetic as syn
    from cosypose_amd.pose_forward_loss import add_noise
    g = dict(np.load(REPO / 'tests' / 'golden' / 'reference_golden_noise.npz'))
    for name in ('gt_noise', 'trans_only', 'one'):
        seed, np_seed, B = (int(v) for v in g[f'{name}_seed'])
        TCO = torch.from_numpy(syn.make_TCO(seed, B))
        np.random.seed(np_seed)
        out = add_noise(TCO, euler_deg_std=list(g[f'{name}_euler_std']), trans_std=list(g[f'{name}_trans_std']))
        assert out.dtype == torch.float32 and tuple(out.shape) == (B, 4, 4)
        np.testing.assert_allclose(out.numpy(), g[f'{name}_out'], rtol=0, atol=2e-7)
        assert np.random.normal() == g[f'{name}_next_draw'][0]
        assert torch.equal(out[:, 3], TCO[:, 3])


def test_shading_fit_recovers_known_constants(oracle):
    """tests/golden/fit_renderer_shading.py fits the rasteriser's 'opengl' shading constants to PyBullet renders (the one part of
    SURVEY 8f-1 that stays parity-unpinned until a box with PyBullet runs it).  The fitter itself is tested here without
    PyBullet: targets rendered by the CPU twin with hidden constants must be recovered."""
    import importlib.util
    import numpy as np
    from conftest import REPO
    spec = importlib.util.spec_from_file_location('fit_renderer_shading', REPO / 'tests' / 'golden' / 'fit_renderer_shading.py')
    F = importlib.util.module_from_spec(spec); spec.loader.exec_module(F)
    scene = F.make_scene(3, n_obj=2, n_poses=4, H=48, W=48)
    hidden = dict(ambient=0.31, diffuse=0.74, specular=0.0, shininess=20.0, light_theta=0.5, light_phi=0.8)
    rgb, mask = F.render_twin(scene, hidden)
    assert mask.mean() > 0.1
    got = F.fit(scene, rgb, mask, x0=[0.4, 0.6, 0.0, 20.0, 0.3, 0.3], maxiter=250)
    assert got['mse'] < 2e-5, got
    assert abs(got['ambient'] - hidden['ambient']) < 0.03 and abs(got['diffuse'] - hidden['diffuse']) < 0.05, got
    want = F.light_dir(hidden['light_theta'], hidden['light_phi'])
    assert float(np.dot(got['light_dir'], want)) > 0.98, got


def test_training_scheduling_helpers_on_the_host():
    """training.LazyMeters keeps the order of the values it is given (CPU values are added at once, behind whatever is still pending),
    mesh_db.select gathers the same rows as indexing with the label list did, train_engine's name-table cache notices a parameter / buffer
    registered anywhere, and DevicePrefetcher refuses to run without a GPU (the product has no CPU path)."""
    import types
    import pytest
    from cosypose_amd import training, train_engine
    from cosypose_amd.mesh_db import BatchedMeshes
    m = training.LazyMeters()
    m.defer([('a',), ('b', 'c')], torch.tensor([1.0, 2.0]))
    m.defer([('a',)], torch.tensor([3.0]))
    m.flush()
    assert m['a'].n == 2 and m['a'].mean == 2.0 and m['b'].mean == 2.0 and m['c'].mean == 2.0
    labels = np.array(['x', 'y', 'z'])
    db = BatchedMeshes({l: dict(label=l, n_points=4, n_sym=1) for l in labels}, labels, torch.rand(3, 4, 3),
                       torch.eye(4).reshape(1, 1, 4, 4).repeat(3, 2, 1, 1) * torch.arange(1, 4).view(3, 1, 1, 1))
    sel = db.select(['z', 'x', 'z'])
    assert torch.equal(sel.points, db.points[[2, 0, 2]]) and torch.equal(sel.symmetries, db.symmetries[[2, 0, 2]]) and list(sel.labels) == ['z', 'x', 'z']
    from cosypose_amd import _modwatch
    before = _modwatch.registration_epoch()
    lin = torch.nn.Linear(2, 2)
    lin.register_buffer('extra', torch.zeros(1))
    assert _modwatch.registration_epoch() >= before + 3          # weight, bias, buffer
    p1, b1 = _modwatch.named_tensors(lin)
    assert _modwatch.named_tensors(lin)[0] is p1                 # cached
    lin.double()                                                 # Module._apply swaps the buffer object without registering: the sentinel sees it
    p2, b2 = _modwatch.named_tensors(lin)
    assert b2['extra'] is lin.extra and b2['extra'].dtype == torch.float64 and p2['weight'] is lin.weight
    lin.more = torch.nn.Parameter(torch.zeros(1))
    assert 'more' in _modwatch.named_tensors(lin)[0]
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match='no GPU'):
            training.DevicePrefetcher([types.SimpleNamespace(images=torch.zeros(1))])


def test_predictor_accepts_models_with_the_reference_forward_signature():
    """A coarse / refiner pair may mix this package's PosePredictor with any module that has the REFERENCE's forward signature
    (models/pose.py:89: images, K, labels, TCO, n_iterations): the package's extensions (`frames_nhwc4=`, `out=`, concurrent lanes) are only used
    with models that take them -- a foreign model runs the sequential path also under n_streams > 1 (round 4's advisor finding: TypeError)."""
    import pandas as pd
    import torch
    from cosypose_amd import tensor_collection as tc
    from cosypose_amd.pose_predictor import CoarseRefinePosePredictor

    class Foreign(torch.nn.Module):
        calls = 0

        def forward(self, images, K, labels, TCO, n_iterations=1, im_ids=None):
            Foreign.calls += 1
            out, cur = {}, TCO
            for n in range(1, n_iterations + 1):
                nxt = cur.clone(); nxt[:, 2, 3] += 0.125
                B = len(labels)
                out[f'iteration={n}'] = dict(TCO_input=cur, TCO_output=nxt, K_crop=K[torch.as_tensor(im_ids)], model_outputs={},
                                             boxes_rend=torch.zeros(B, 4), boxes_crop=torch.ones(B, 4))
                cur = nxt
            return out

    D = 5
    infos = pd.DataFrame(dict(label=[f'o{i}' for i in range(D)], batch_im_id=[0, 1, 0, 1, 0], score=1.0))
    init = tc.PandasTensorCollection(infos=infos, poses=torch.eye(4).repeat(D, 1, 1))
    images, K = torch.zeros(2, 3, 8, 8), torch.eye(3).repeat(2, 1, 1)
    for n_streams in (1, 2):
        pred = CoarseRefinePosePredictor(coarse_model=None, refiner_model=Foreign(), bsz_objects=2, n_streams=n_streams)
        final, allp = pred.get_predictions(images, K, data_TCO_init=init, n_coarse_iterations=0, n_refiner_iterations=2)
        assert list(allp) == ['external_coarse', 'refiner/iteration=1', 'refiner/iteration=2']
        assert torch.equal(final.poses[:, 2, 3], torch.full((D,), 0.25)) and len(final) == D
    assert Foreign.calls == 6 and not CoarseRefinePosePredictor._accepts(Foreign(), 'out')
    from cosypose_amd.pose import PosePredictor
    assert CoarseRefinePosePredictor._accepts(PosePredictor.__new__(PosePredictor), 'out')


def test_bench_dump_outputs_writes_float32_arrays_within_the_cap(tmp_path):
    """bench.py --dump-outputs: the step's poses and every stage / iteration field as <name>.npy in float32 (16-bit fields widened), the given
    initial poses of config 2 left out; above the byte cap every array keeps the same seeded, sorted rows, so two runs write the same files."""
    import bench
    from cosypose_amd import tensor_collection as tc
    n = 64
    g = torch.Generator().manual_seed(0)
    infos = pd.DataFrame(dict(label=['obj_1'] * n, batch_im_id=0, score=1.0))
    preds = {'external_coarse': tc.PandasTensorCollection(infos, poses=torch.rand(n, 4, 4, generator=g)),
             'refiner/iteration=1': tc.PandasTensorCollection(infos, poses=torch.rand(n, 4, 4, generator=g), K_crop=torch.rand(n, 3, 3, generator=g),
                                                              boxes_crop=torch.rand(n, 4, generator=g).half())}
    poses = torch.rand(n, 4, 4, generator=g)
    bench.dump_outputs(tmp_path / 'all', poses, preds)
    got = {p.stem: np.load(p) for p in (tmp_path / 'all').iterdir()}
    assert sorted(got) == ['poses', 'refiner_iteration1_K_crop', 'refiner_iteration1_boxes_crop', 'refiner_iteration1_poses']
    assert all(a.dtype == np.float32 and len(a) == n for a in got.values())
    assert np.array_equal(got['poses'], poses.numpy())
    assert np.array_equal(got['refiner_iteration1_boxes_crop'], preds['refiner/iteration=1'].boxes_crop.float().numpy())
    cap = 4096
    for d in ('a', 'b'):
        bench.dump_outputs(tmp_path / d, poses, preds, limit=cap)
    a = {p.stem: np.load(p) for p in (tmp_path / 'a').iterdir()}
    b = {p.stem: np.load(p) for p in (tmp_path / 'b').iterdir()}
    assert sum(v.nbytes for v in a.values()) <= cap and 0 < len(a['poses']) < n
    assert all(np.array_equal(a[k], b[k]) for k in a)
    rows = [i for i in range(n) if any(np.array_equal(poses.numpy()[i], r) for r in a['poses'])]
    assert np.array_equal(a['poses'], poses.numpy()[rows])        # whole rows, in their order
