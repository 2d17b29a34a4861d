"""Seeded synthetic inputs for parity tests and bench.py.

Everything is generated with numpy's legacy ``RandomState`` (bit-stable across
numpy versions and machines), so the build container and the GPU box produce
identical tensors from a seed and golden fixtures only need to hold outputs.
"""
import numpy as np

# (k, s, expand, cin, cout) per MBConv block of EfficientNet-B3 with 6 input
# channels, as instantiated by EfficientNet.from_name('efficientnet-b3', in_channels=6)
# (reference cosypose/training/pose_models_cfg.py:23; block strings
# cosypose/models/efficientnet_utils.py:259-264).  Derived, not copied:
# see cosypose_amd.efficientnet.b3_block_table().
from .arch import B3_BLOCKS, STEM_C, HEAD_C, IN_C, N_POSE


def state_dict_shapes(prefix='backbone.'):
    """Ordered {key: shape} of the reference PosePredictor state_dict (sans num_batches_tracked)."""
    out = {}

    def bn(p, c):
        for s in ('weight', 'bias', 'running_mean', 'running_var'):
            out[f'{p}.{s}'] = (c,)
    out[prefix + '_conv_stem.weight'] = (STEM_C, IN_C, 3, 3)
    bn(prefix + '_bn0', STEM_C)
    for i, (k, s, e, cin, cout) in enumerate(B3_BLOCKS):
        p = f'{prefix}_blocks.{i}.'
        cmid = cin * e
        cse = max(1, int(cin * 0.25))
        if e != 1:
            out[p + '_expand_conv.weight'] = (cmid, cin, 1, 1)
            bn(p + '_bn0', cmid)
        out[p + '_depthwise_conv.weight'] = (cmid, 1, k, k)
        bn(p + '_bn1', cmid)
        out[p + '_se_reduce.weight'] = (cse, cmid, 1, 1)
        out[p + '_se_reduce.bias'] = (cse,)
        out[p + '_se_expand.weight'] = (cmid, cse, 1, 1)
        out[p + '_se_expand.bias'] = (cmid,)
        out[p + '_project_conv.weight'] = (cout, cmid, 1, 1)
        bn(p + '_bn2', cout)
    out[prefix + '_conv_head.weight'] = (HEAD_C, 384, 1, 1)
    bn(prefix + '_bn1', HEAD_C)
    out['pose_fc.weight'] = (N_POSE, HEAD_C)
    out['pose_fc.bias'] = (N_POSE,)
    return out


def golden_state_dict(seed=0):
    """Well-conditioned random weights (SURVEY 8c "Golden weights"): variance-preserving
    convs, randomised BN statistics, and a pose head with small weights and bias
    [1,0,0, 0,1,0, 0,0,1] so that dR ~ I and (vx,vy,vz) ~ (0,0,1): poses stay finite
    over many iterations.  Returns {key: np.float32 array}."""
    rs = np.random.RandomState(seed)
    sd = {}
    for k, shp in state_dict_shapes().items():
        if k.endswith('running_var'):
            v = rs.uniform(0.5, 1.5, shp)
        elif k.endswith('running_mean'):
            v = rs.normal(0, 0.1, shp)
        elif '_bn' in k and k.endswith('.weight'):
            v = rs.uniform(0.7, 1.3, shp)
        elif '_bn' in k and k.endswith('.bias'):
            v = rs.normal(0, 0.1, shp)
        elif k == 'pose_fc.weight':
            v = rs.normal(0, 1.0 / np.sqrt(HEAD_C), shp) * 1e-2
        elif k == 'pose_fc.bias':
            v = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], np.float64)
        elif k.endswith('.bias'):
            v = rs.normal(0, 0.1, shp)
        else:  # conv weight (O, I/groups, kh, kw)
            fan_in = shp[1] * shp[2] * shp[3]
            v = rs.normal(0, np.sqrt(1.8 / fan_in), shp)
        sd[k] = np.ascontiguousarray(v, dtype=np.float32)
    return sd


def make_frames(seed, n, h, w):
    """(n,3,h,w) uniform [0,1) fp32 frames."""
    return np.random.RandomState(seed).random_sample((n, 3, h, w)).astype(np.float32)


def make_K(n, h, w):
    """fx=fy=1066.8*(w/640), cx=w/2-7, cy=h/2+1.3 (YCB-V-like)."""
    K = np.zeros((n, 3, 3), np.float32)
    K[:, 0, 0] = K[:, 1, 1] = 1066.8 * (w / 640.0)
    K[:, 0, 2] = w / 2.0 - 7.0
    K[:, 1, 2] = h / 2.0 + 1.3
    K[:, 2, 2] = 1.0
    return K


def make_mesh_points(seed, n_obj, n_pts=2500):
    """(n_obj, n_pts, 3) points uniform in a box of half-extent U(0.03,0.12) m per axis."""
    rs = np.random.RandomState(seed)
    ext = rs.uniform(0.03, 0.12, (n_obj, 1, 3))
    pts = rs.uniform(-1, 1, (n_obj, n_pts, 3)) * ext
    return pts.astype(np.float32)


def make_detections(seed, n_det, n_frames, n_obj, h, w):
    """label ids (n_det,), batch_im_id (n_det,), bboxes (n_det,4): centre in the central
    60% of the frame, side U(60,220) px."""
    rs = np.random.RandomState(seed)
    obj = rs.randint(0, n_obj, n_det)
    im = rs.randint(0, n_frames, n_det)
    cx = rs.uniform(0.2 * w, 0.8 * w, n_det); cy = rs.uniform(0.2 * h, 0.8 * h, n_det)
    sw = rs.uniform(60, 220, n_det) * (min(h, w) / 480.0); sh = rs.uniform(60, 220, n_det) * (min(h, w) / 480.0)
    boxes = np.stack([cx - sw / 2, cy - sh / 2, cx + sw / 2, cy + sh / 2], 1).astype(np.float32)
    return obj.astype(np.int64), im.astype(np.int64), boxes


def make_TCO(seed, n, z_range=(0.6, 1.4), xy=0.15):
    """(n,4,4) random well-conditioned object poses in front of the camera."""
    rs = np.random.RandomState(seed)
    q = rs.normal(size=(n, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
    w_, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w_), 2 * (x * z + y * w_),
                  2 * (x * y + z * w_), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w_),
                  2 * (x * z - y * w_), 2 * (y * z + x * w_), 1 - 2 * (x * x + y * y)], 1).reshape(n, 3, 3)
    T = np.tile(np.eye(4), (n, 1, 1))
    T[:, :3, :3] = R
    T[:, 0, 3] = rs.uniform(-xy, xy, n); T[:, 1, 3] = rs.uniform(-xy, xy, n); T[:, 2, 3] = rs.uniform(*z_range, n)
    return T.astype(np.float32)


def make_renders(seed, n, H, W):
    """Deterministic stand-in for renderer.render: (n,3,H,W) in [0,1)."""
    return np.random.RandomState(seed).random_sample((n, 3, H, W)).astype(np.float32)


def make_training_batch(seed, B, n_obj=21, h=480, w=640):
    """One synthetic training batch: uint8 frames (B,3,h,w), K (B,3,3), ground-truth
    poses (B,4,4) and object ids (B,)."""
    frames = (make_frames(seed, B, h, w) * 255).astype(np.uint8)
    K = make_K(B, h, w)
    TCO = make_TCO(seed + 1, B)
    obj = np.random.RandomState(seed + 2).randint(0, n_obj, B).astype(np.int32)
    return frames, K, TCO, obj


def make_render_meshes(seed, n_obj, n_lat=24, n_lon=32):
    """Closed triangle meshes for the rasteriser: bumpy ellipsoids with the half-extents make_mesh_points(seed, ...) draws
    (so that geometry points and render meshes describe the same objects) and smooth vertex colours.
    -> verts list [(V,3)], faces list [(F,3) int32], colors list [(V,3)]"""
    rs = np.random.RandomState(seed)
    ext = rs.uniform(0.03, 0.12, (n_obj, 1, 3))
    rs = np.random.RandomState(seed + 1000)
    lat = np.linspace(0, np.pi, n_lat + 1)[1:-1]
    lon = np.linspace(0, 2 * np.pi, n_lon, endpoint=False)
    verts_l, faces_l, colors_l = [], [], []
    ring = lambda i: 1 + i * n_lon
    faces = []
    for j in range(n_lon):
        faces.append((0, ring(0) + j, ring(0) + (j + 1) % n_lon))
    for i in range(len(lat) - 1):
        for j in range(n_lon):
            a, b = ring(i) + j, ring(i) + (j + 1) % n_lon
            c, d = ring(i + 1) + j, ring(i + 1) + (j + 1) % n_lon
            faces += [(a, c, b), (b, c, d)]
    south = 1 + len(lat) * n_lon
    for j in range(n_lon):
        faces.append((south, ring(len(lat) - 1) + (j + 1) % n_lon, ring(len(lat) - 1) + j))
    faces = np.asarray(faces, np.int32)
    for o in range(n_obj):
        dirs = [np.array([0, 0, 1.0])]
        for t in lat:
            for p in lon:
                dirs.append(np.array([np.sin(t) * np.cos(p), np.sin(t) * np.sin(p), np.cos(t)]))
        dirs.append(np.array([0, 0, -1.0]))
        dirs = np.asarray(dirs)
        f = rs.uniform(1, 3, 3); ph = rs.uniform(0, 6.28, 3)
        bump = 1 + 0.15 * np.sin(f[0] * dirs[:, 0] * 3 + ph[0]) * np.cos(f[1] * dirs[:, 1] * 3 + ph[1]) + 0.1 * np.sin(f[2] * dirs[:, 2] * 4 + ph[2])
        verts_l.append((dirs * bump[:, None] * ext[o]).astype(np.float32))
        base = rs.uniform(0.2, 0.9, 3)
        colors_l.append(np.clip(base + 0.3 * dirs * rs.uniform(-1, 1, 3), 0, 1).astype(np.float32))
        faces_l.append(faces)
    return verts_l, faces_l, colors_l


# ---- multi-view scenes for the bundle adjustment (cosypose_amd/bundle_adjustment.py) ----------------------------------------
BA_N_SYM = (1, 2, 4, 3)     # real symmetries of the four synthetic meshes (rotations about z), identity-padded to S = 4


def _rodrigues(rs, angle_std):
    """rotation by N(0, angle_std) radians about a random axis"""
    axis = rs.randn(3)
    axis /= np.linalg.norm(axis)
    a = rs.randn() * angle_std
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * (Kx @ Kx)


def _rigid_noise(rs, angle_std, trans_std):
    T = np.eye(4)
    T[:3, :3] = _rodrigues(rs, angle_std)
    T[:3, 3] = rs.randn(3) * trans_std
    return T


def make_ba_scene(seed, n_objects, n_views, n_points, exact_pairs=False, p_visible=0.75):
    """A seeded multi-view scene, float64: objects standing on a table, cameras on a 0.9 m hemisphere looking at the origin
    (600 px focal, 640x480), per-view candidates = true pose . a random symmetry of the mesh . noise (0.03 rad, 4 mm), all
    ordered view pairs with relative poses noisy by 0.02 rad / 5 mm (or exact).  n_points == 8 gives the corners of each mesh's
    bounding box.  -> dict of numpy arrays: the mesh tables (pts, sym, n_sym), the candidates' columns (cand_view_id, cand_obj_id,
    cand_label_id, cand_score, cand_poses), the cameras' (cam_view_id, cam_K, cam_TWC: the truth) and the pairs' (pair_view1,
    pair_view2, pair_TC1C2)."""
    rs = np.random.RandomState(seed)
    n_mesh, S = len(BA_N_SYM), max(BA_N_SYM)
    ext = rs.uniform(0.03, 0.12, (n_mesh, 1, 3))
    if n_points == 8:
        corners = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float64)
        pts = corners[None] * ext
    else:
        pts = rs.uniform(-1, 1, (n_mesh, n_points, 3)) * ext
    sym = np.tile(np.eye(4), (n_mesh, S, 1, 1))
    for m in range(n_mesh):
        for k in range(1, BA_N_SYM[m]):
            a = 2 * np.pi * k / BA_N_SYM[m]
            sym[m, k, :3, :3] = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    obj_mesh = rs.randint(0, n_mesh, n_objects)
    TWO = np.tile(np.eye(4), (n_objects, 1, 1))
    for o in range(n_objects):
        a = rs.uniform(0, 2 * np.pi)
        TWO[o, :3, :3] = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        TWO[o, :3, 3] = [rs.uniform(-0.25, 0.25), rs.uniform(-0.25, 0.25), ext[obj_mesh[o], 0, 2]]
    TWC = np.tile(np.eye(4), (n_views, 1, 1))
    for v in range(n_views):
        az, el = rs.uniform(0, 2 * np.pi), rs.uniform(np.radians(25), np.radians(75))
        c = 0.9 * np.array([np.cos(az) * np.cos(el), np.sin(az) * np.cos(el), np.sin(el)])
        z = -c / np.linalg.norm(c)                       # optical axis: towards the origin
        x = np.cross(z, [0., 0., 1.]); x /= np.linalg.norm(x)
        TWC[v, :3, :3] = np.stack([x, np.cross(z, x), z], axis=1)
        TWC[v, :3, 3] = c
    TCW = np.linalg.inv(TWC)
    visible = rs.uniform(size=(n_objects, n_views)) < p_visible
    for o in range(n_objects):                           # every object is seen at least once, every view sees something
        if not visible[o].any():
            visible[o, rs.randint(n_views)] = True
    for v in range(n_views):
        if not visible[:, v].any():
            visible[rs.randint(n_objects), v] = True
    view_ids, obj_ids = 10 + 3 * np.arange(n_views), 100 + np.arange(n_objects)
    cv, co, cl, cp = [], [], [], []
    for v in range(n_views):
        for o in range(n_objects):
            if visible[o, v]:
                m = obj_mesh[o]
                cv.append(view_ids[v]); co.append(obj_ids[o]); cl.append(m)
                cp.append(TCW[v] @ TWO[o] @ sym[m, rs.randint(BA_N_SYM[m])] @ _rigid_noise(rs, 0.03, 0.004))
    p1, p2, pt = [], [], []
    for a in range(n_views):
        for b in range(n_views):
            if a != b:
                T = TCW[a] @ TWC[b]
                p1.append(view_ids[a]); p2.append(view_ids[b])
                pt.append(T if exact_pairs else T @ _rigid_noise(rs, 0.02, 0.005))
    K = np.tile(np.array([[600., 0, 320], [0, 600., 240], [0, 0, 1]]), (n_views, 1, 1))
    return dict(pts=pts, sym=sym, n_sym=np.array(BA_N_SYM, np.int32), cand_view_id=np.array(cv, np.int64), cand_obj_id=np.array(co, np.int64),
                cand_label_id=np.array(cl, np.int64), cand_score=rs.uniform(0.5, 1.0, len(cv)), cand_poses=np.array(cp),
                cam_view_id=view_ids.astype(np.int64), cam_K=K, cam_TWC=TWC, pair_view1=np.array(p1, np.int64),
                pair_view2=np.array(p2, np.int64), pair_TC1C2=np.array(pt).reshape(-1, 4, 4))


def ba_scene_collections(scene, make_mesh_db, dtype=None, device=None, collection=None):
    """(candidates, cameras, pairs_TC1C2, mesh_db) of a make_ba_scene dict (or the same columns loaded from a fixture) as
    PandasTensorCollections.  `make_mesh_db(infos, labels, points, symmetries)` is the BatchedMeshes class to use, `collection` the
    PandasTensorCollection class (default: this package's)."""
    import pandas as pd
    import torch
    if collection is None:
        from .tensor_collection import PandasTensorCollection as collection
    PandasTensorCollection = collection
    dtype = dtype or torch.float64

    def t(a):
        out = torch.as_tensor(np.asarray(a)).to(dtype)
        return out.to(device) if device is not None else out
    labels = np.array([f'obj_{i:06d}' for i in range(1, len(scene['n_sym']) + 1)])
    infos = {l: dict(label=l, n_points=scene['pts'].shape[1], n_sym=int(scene['n_sym'][i])) for i, l in enumerate(labels)}
    mesh_db = make_mesh_db(infos, labels, t(scene['pts']), t(scene['sym']))
    cand = PandasTensorCollection(pd.DataFrame(dict(view_id=scene['cand_view_id'], obj_id=scene['cand_obj_id'],
                                                    label=labels[scene['cand_label_id']], score=scene['cand_score'])), poses=t(scene['cand_poses']))
    cams = PandasTensorCollection(pd.DataFrame(dict(view_id=scene['cam_view_id'])), K=t(scene['cam_K']))
    pairs = PandasTensorCollection(pd.DataFrame(dict(view1=scene['pair_view1'], view2=scene['pair_view2'])), TC1C2=t(scene['pair_TC1C2']))
    return cand, cams, pairs, mesh_db


# ---- evaluation scenes for the pose meter (cosypose_amd/pose_meters.py) -------------------------------------------------------------
EVAL_N_POINTS = (150, 257, 400, 640, 900, 1100, 1500)      # points per label: all different, one just past a 256-point boundary


def make_eval_meshes(seed, n_points=EVAL_N_POINTS):
    """Meshes of different sizes for the pose meter -> (labels, points (n_obj, max n, 3) float32 padded by repeating each mesh's first
    point, infos {label: dict(label, n_points, n_sym, is_symmetric, diameter_m)}).  Every second label is symmetric; the diameter is
    the diagonal of the bounding box."""
    rs = np.random.RandomState(seed)
    labels = [f'obj_{n + 1:06d}' for n in range(len(n_points))]
    pts = np.zeros((len(labels), max(n_points), 3), dtype=np.float32)
    infos = {}
    for n, (label, P) in enumerate(zip(labels, n_points)):
        ext = rs.uniform(0.03, 0.12, 3)
        p = (rs.uniform(-1, 1, (P, 3)) * ext).astype(np.float32)
        pts[n, :P] = p
        pts[n, P:] = p[0]
        diameter = float(np.linalg.norm(p.max(0).astype(np.float64) - p.min(0).astype(np.float64)))
        infos[label] = dict(label=label, n_points=P, n_sym=1, is_symmetric=bool(n % 2), diameter_m=diameter)
    return labels, pts, infos


def make_eval_scene(seed, labels, infos, scene_ids=(3, 7), n_views=3):
    """Ground truth and predictions of a few views for the pose meter -> dict of columns (numpy): gt_scene_id, gt_view_id, gt_label
    (index into labels), gt_visib_fract, gt_poses (n,4,4) float32; pred_scene_id, pred_view_id, pred_label, pred_score (all
    different), pred_poses.  Up to three instances of a label per view, the later ones within a diameter of the first; a
    prediction per ground truth with probability 0.85, noisy by 0.5 % / 4 % / 12 % / 40 % of the diameter (and 0.01-0.3 rad), plus
    spurious predictions, predictions of labels that are not in the view and predictions in a view without ground truth."""
    rs = np.random.RandomState(seed)
    gt, pred = [], []
    for scene_id in scene_ids:
        for view_id in range(n_views):
            present = rs.permutation(len(labels))[:rs.randint(4, len(labels) + 1)]
            for l in present:
                d = infos[labels[l]]['diameter_m']
                base = make_TCO(rs.randint(1 << 30), 1)[0].astype(np.float64)
                for inst in range(rs.randint(1, 4)):
                    T = base.copy()
                    if inst:
                        T = T @ _rigid_noise(rs, 1.0, 0.35 * d)
                    gt.append((scene_id, view_id, l, rs.uniform(0.05, 1.0), T))
                    if rs.uniform() < 0.85:
                        level = rs.randint(4)
                        noise = _rigid_noise(rs, (0.01, 0.05, 0.15, 0.3)[level], (0.005, 0.04, 0.12, 0.4)[level] * d / np.sqrt(3))
                        pred.append((scene_id, view_id, l, T @ noise))
                if rs.uniform() < 0.3:      # a spurious prediction near the object
                    pred.append((scene_id, view_id, l, base @ _rigid_noise(rs, 1.0, 0.5 * d)))
            absent = [l for l in range(len(labels)) if l not in present]
            if absent:                      # a label the view does not hold
                pred.append((scene_id, view_id, absent[0], make_TCO(rs.randint(1 << 30), 1)[0].astype(np.float64)))
    pred.append((scene_ids[0], n_views + 5, 0, make_TCO(rs.randint(1 << 30), 1)[0].astype(np.float64)))      # a view without ground truth
    order = rs.permutation(len(pred))
    pred = [pred[n] for n in order]
    score = rs.permutation(len(pred)).astype(np.float64) / len(pred) * 0.9 + 0.05
    return dict(gt_scene_id=np.array([g[0] for g in gt]), gt_view_id=np.array([g[1] for g in gt]), gt_label=np.array([g[2] for g in gt]),
                gt_visib_fract=np.array([g[3] for g in gt]), gt_poses=np.stack([g[4] for g in gt]).astype(np.float32),
                pred_scene_id=np.array([p[0] for p in pred]), pred_view_id=np.array([p[1] for p in pred]),
                pred_label=np.array([p[2] for p in pred]), pred_score=score, pred_poses=np.stack([p[3] for p in pred]).astype(np.float32))


# ---- detection scenes for the detection meter (cosypose_amd/detection_meters.py) and instance masks (cosypose_amd/mask_ops.py) -------
def make_det_scene(seed, n_labels=6, scene_ids=(3, 7), n_views=3):
    """Ground-truth and predicted boxes of a few views for the detection meter -> dict of columns (numpy): gt_scene_id, gt_view_id,
    gt_label (index below n_labels), gt_visib_fract, gt_bboxes (n,4) float32 xyxy; pred_scene_id, pred_view_id, pred_label,
    pred_score (all different), pred_bboxes.  One to three instances of a label per view, all around one base box (so the boxes of
    a (scene, view, label) group overlap one another); a prediction per ground truth with probability 0.85, jittered by up to 1 % /
    5 % / 15 % / 30 % of the box size, sometimes a duplicate of it, plus false positives near the group, predictions of labels that
    are not in the view and one in a view without ground truth.  The LAST label has one instance per view and predictions shifted by
    30-40 % of the box along both axes: it never has a true positive at an IoU threshold of 0.5."""
    rs = np.random.RandomState(seed)
    gt, pred = [], []

    def moved(box, shift, scale):
        cx, cy, w, h = (box[0] + box[2]) / 2, (box[1] + box[3]) / 2, box[2] - box[0], box[3] - box[1]
        cx, cy = cx + shift[0] * w, cy + shift[1] * h
        w, h = w * scale[0], h * scale[1]
        return np.array([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2])

    for scene_id in scene_ids:
        for view_id in range(n_views):
            present = rs.permutation(n_labels - 1)[:rs.randint(3, n_labels)].tolist() + [n_labels - 1]
            for l in present:
                w, h = rs.uniform(60, 160, 2)
                x, y = rs.uniform(0, 640 - w), rs.uniform(0, 480 - h)
                base = np.array([x, y, x + w, y + h])
                if l == n_labels - 1:
                    gt.append((scene_id, view_id, l, rs.uniform(0.05, 1.0), base))
                    sign = rs.choice([-1., 1.], 2)
                    pred.append((scene_id, view_id, l, moved(base, sign * rs.uniform(0.3, 0.4, 2), (1., 1.))))
                    continue
                for inst in range(rs.randint(1, 4)):
                    box = moved(base, rs.uniform(-0.2, 0.2, 2), rs.uniform(0.9, 1.1, 2)) if inst else base
                    gt.append((scene_id, view_id, l, rs.uniform(0.05, 1.0), box))
                    if rs.uniform() < 0.85:
                        level = (0.01, 0.05, 0.15, 0.3)[rs.randint(4)]
                        pred.append((scene_id, view_id, l, moved(box, rs.uniform(-level, level, 2), 1 + rs.uniform(-level, level, 2) / 3)))
                        if rs.uniform() < 0.25:      # a duplicate detection of the same object
                            pred.append((scene_id, view_id, l, moved(box, rs.uniform(-0.05, 0.05, 2), 1 + rs.uniform(-0.02, 0.02, 2))))
                if rs.uniform() < 0.4:               # a false positive near the group
                    pred.append((scene_id, view_id, l, moved(base, rs.uniform(-0.4, 0.4, 2), rs.uniform(0.9, 1.1, 2))))
            absent = [l for l in range(n_labels) if l not in present]
            if absent:                               # a label the view does not hold
                pred.append((scene_id, view_id, absent[0], np.array([10., 10., 90., 70.]) + rs.uniform(0, 300)))
    pred.append((scene_ids[0], n_views + 5, 0, np.array([20., 30., 120., 140.])))      # a view without ground truth
    order = rs.permutation(len(pred))
    pred = [pred[n] for n in order]
    score = rs.permutation(len(pred)).astype(np.float64) / len(pred) * 0.9 + 0.05
    return dict(gt_scene_id=np.array([g[0] for g in gt]), gt_view_id=np.array([g[1] for g in gt]), gt_label=np.array([g[2] for g in gt]),
                gt_visib_fract=np.array([g[3] for g in gt]), gt_bboxes=np.stack([g[4] for g in gt]).astype(np.float32),
                pred_scene_id=np.array([p[0] for p in pred]), pred_view_id=np.array([p[1] for p in pred]),
                pred_label=np.array([p[2] for p in pred]), pred_score=score, pred_bboxes=np.stack([p[3] for p in pred]).astype(np.float32))


def make_instance_masks(seed, B, H, W, n_inst):
    """(B,H,W) uint8 instance-id masks: background 0, then instances 1..n_inst drawn in that order (a later one covers an earlier one),
    alternately axis-aligned rectangles and ellipses of random place and size; some end up partly or wholly covered, some cut by the frame."""
    rs = np.random.RandomState(seed)
    masks = np.zeros((B, H, W), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    for b in range(B):
        for n in range(1, n_inst + 1):
            cx, cy = rs.uniform(0, W), rs.uniform(0, H)
            rx, ry = rs.uniform(0.02, 0.2) * W + 0.5, rs.uniform(0.02, 0.2) * H + 0.5
            x0, x1 = max(int(cx - rx), 0), min(int(cx + rx) + 1, W)
            y0, y1 = max(int(cy - ry), 0), min(int(cy + ry) + 1, H)
            if n % 2:
                masks[b, y0:y1, x0:x1] = n
            else:
                win = (slice(y0, y1), slice(x0, x1))
                inside = ((xx[win] - cx) / rx) ** 2 + ((yy[win] - cy) / ry) ** 2 <= 1.
                masks[b][win][inside] = n
    return masks
