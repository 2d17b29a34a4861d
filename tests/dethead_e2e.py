"""The seeded 2-frame case of the end-to-end test of the detector's heads (tests/test_detector_heads.py) and, computed on the CPU alone from
the twins detpre_ref / detpost_ref and the heads' float64 values and running bounds (dethead_ref), the MARGIN of every decision the chain
takes: how far its value lies from its threshold, in units of what the heads' bound can move that value.  The test asserts margin > 100.

Two runs are compared on the device: detections_from_features with DetectorHeads, and with the same layers as torch.nn modules.  Each head
output of either run lies within the running bound e of the float64 value (any order of float32 additions meets (K + 2) u S), so a decision
whose value is further than its bound from the threshold falls the same way in both.  What moves with the head outputs, and by how much:
  * RPN.  The box deltas' weights and biases are ZERO in this case: both runs decode exactly the anchors, proposals are bit-equal, and the
    IoUs of the RPN's NMS are the same numbers in both runs.  (The delta columns with real weights are held to the bit by the layer tests.)
    Left are the objectness logits s +- e: the top-k boundary of a level, and the order of every pair of candidates of one level whose
    IoU exceeds the NMS threshold (greedy NMS depends on the scores only through the order inside such pairs).
  * Box head on bit-equal RoI features: class logits +- eps give softmax scores s (1 +- (exp(2 eps) - 1)); regression +- e_r gives the
    corners +- delta = w (e_dx / 10) + 0.5 w exp(dw / 5) (exp(e_dw / 5) - 1) (+ 8 float32 ulps of the coordinate for the device's own
    roundings).  Decisions: score against score_thresh; sides against the small-box limit; per class the IoU of every pair against nms_thresh,
    where corners moved by t change intersection and union by at most dI = 2 t (iw + ih) + 4 t^2 and dU = dA1 + dA2 + dI and so the IoU by
    (dI + IoU dU) / (U - dU); the order of every pair whose IoU can exceed the threshold; detections_per_img is not reached.
  * Masks: the final boxes differ by delta between the runs, so the 14 x 14 RoI features differ by at most 12 max|f| scale delta (a bilinear
    sample moves by at most 3 scale delta per axis over cells that differ by at most 2 max|f|), which enters the mask head's running bound as
    err0; a pasted probability moves by at most a quarter of the logit's bound.  Decisions: every edge of the expanded box against the
    integers it is truncated at, every pasted pixel against mask_th.
Not modelled: RoIAlign's cut of samples outside [-1, size] (the boxes are clipped to the image, whose cells the maps cover)."""
import functools

import numpy as np
import torch

import dethead_case as case
import dethead_ref as ref
import detpost_ref as post
import detpre_ref as pre

F32 = np.float32
GRID = [(5, 7), (3, 4), (1, 2)]
SIZES = ((8,), (16,), (32,))              # anchors that fit the 37 x 53 images: boxes of different levels stay below the NMS threshold
PAD, NETS, FRAME = (40, 56), [(37, 53), (40, 50)], (24, 40)
NAMES = {1: 'obj_000001', 2: 'obj_000002'}
PRE, POST, PER_IMG, SCORE_TH, NMS_TH, RPN_NMS_TH, MASK_TH = 1, 1000, 100, 0.05, 0.5, 0.7, 0.8
SEED = 10                                  # chosen on the CPU by search() below: the first seed whose every margin exceeds 100


@functools.lru_cache(maxsize=None)
def weights(seed):
    rng = np.random.RandomState(1000 + seed)
    C, A, K, sd = case.CHAIN_C, case.A, case.K, {}

    def put(name, shape, scale, bias=0.1):
        sd[name + '.weight'] = (rng.normal(0, 1, shape) * scale).astype(F32)
        sd[name + '.bias'] = (rng.normal(0, 1, shape[1] if 'conv5_mask' in name else shape[0]) * bias).astype(F32)
    put('rpn.head.conv', (C, C, 3, 3), 0.3)
    put('rpn.head.cls_logits', (A, C, 1, 1), 0.5)
    put('rpn.head.bbox_pred', (4 * A, C, 1, 1), 0.0, 0.0)              # zero: see the module's docstring
    put('roi_heads.box_head.fc6', (16, C * 49), 0.3 / 7, 0.05)
    put('roi_heads.box_head.fc7', (16, 16), 0.15, 0.05)
    put('roi_heads.box_predictor.cls_score', (K, 16), 0.3, 0.3)
    put('roi_heads.box_predictor.bbox_pred', (4 * K, 16), 0.005, 0.3)
    for i in range(1, 5):
        put(f'roi_heads.mask_head.mask_fcn{i}', (C, C, 3, 3), 0.02, 0.3)
    put('roi_heads.mask_predictor.conv5_mask', (C, C, 2, 2), 0.2, 0.3)
    put('roi_heads.mask_predictor.mask_fcn_logits', (K, C, 1, 1), 0.3, 1.5)
    sd['roi_heads.mask_predictor.mask_fcn_logits.bias'][1:] += F32(2)      # the object classes' masks are mostly on
    return sd


def features(seed):
    rng = np.random.RandomState(seed)
    return [rng.normal(0, 1, (2, case.CHAIN_C, H, W)).astype(F32) for H, W in GRID]


def iou_move(a, b, t):
    """-> IoU of boxes a, b (float64) and the most it can change when every corner moves by at most t"""
    iw, ih = max(min(a[2], b[2]) - max(a[0], b[0]), 0.0), max(min(a[3], b[3]) - max(a[1], b[1]), 0.0)
    area = lambda q: (q[2] - q[0]) * (q[3] - q[1])
    I, U = iw * ih, area(a) + area(b) - iw * ih
    dI = 2 * t * (iw + ih) + 4 * t * t
    dU = sum(2 * t * ((q[2] - q[0]) + (q[3] - q[1])) + 4 * t * t for q in (a, b)) + dI
    return I / U, ((dI + I / U * dU) / (U - dU) if U > dU else np.inf)


@functools.lru_cache(maxsize=None)
def margins(seed):
    """-> {decision: smallest margin in units of the heads' bound}, and what the test needs of the twin chain"""
    sd, feats = weights(seed), features(seed)
    m = {}

    def note(key, value):
        m[key] = min(m.get(key, np.inf), float(value))
    # ---- RPN: logits s +- e; deltas are exactly zero on every side
    rpn = ref.rpn_head(sd, feats, 'float32')
    assert all(not d.any() and not e.any() for _, _, d, e in rpn)
    obj, dl = [o.astype(F32) for o, _, _, _ in rpn], [d.astype(F32) for _, _, d, _ in rpn]
    props = pre.proposals(obj, dl, NETS, PAD, sizes=SIZES, pre_nms_top_n=PRE, post_nms_top_n=POST)
    for b in range(2):
        for l, (o, e_o, d, _) in enumerate(rpn):
            s, rel = pre.flatten_level(o[b], d[b])
            e = pre.flatten_level(e_o[b], d[b])[0]
            idx = pre.top_k(s.astype(F32), rel.astype(F32), PRE)
            out = np.setdiff1d(np.arange(len(s)), idx)
            if len(out):                                           # the top-k boundary: the lowest taken against the highest left
                i, j = idx[np.argmin(s[idx])], out[np.argmax(s[out])]
                note('rpn top-k', (s[i] - s[j]) / (e[i] + e[j]))
            anc = post.clip(torch.as_tensor(pre.level_anchors(*GRID[l], PAD, SIZES[l])[idx]), NETS[b]).double().numpy()
            for p in range(len(idx)):
                for q in range(p):
                    iou, _ = iou_move(anc[p], anc[q], 0.0)
                    note('rpn nms iou (same numbers in both runs)', np.inf if iou != RPN_NMS_TH else 0.0)
                    if iou > RPN_NMS_TH:
                        note('rpn nms order', abs(s[idx[p]] - s[idx[q]]) / (e[idx[p]] + e[idx[q]]))
        note('rpn post-nms top-n not reached', np.inf if len(props[b]['boxes']) < POST else 0.0)
    # ---- box head on bit-equal RoI features
    scales = pre.infer_scales([f.shape[2:] for f in feats], NETS)
    boxes = np.concatenate([p['boxes'] for p in props]).reshape(-1, 4)
    im = np.concatenate([np.full(len(p['boxes']), b) for b, p in enumerate(props)])
    roi = pre.multiscale_roi_align(feats, boxes, im, scales, 7, 2)[0].astype(F32)
    v_c, e_c, v_r, e_r = ref.box_head(sd, roi, 'float32')
    z = v_c - v_c.max(1, keepdims=True)
    sc = np.exp(z) / np.exp(z).sum(1, keepdims=True)
    d_sc = sc * np.expm1(2 * e_c.max(1, keepdims=True))
    p64 = boxes.astype(np.float64)
    w, h = p64[:, 2] - p64[:, 0], p64[:, 3] - p64[:, 1]
    cx, cy = p64[:, 0] + 0.5 * w, p64[:, 1] + 0.5 * h
    rel, e_rel = v_r.reshape(len(boxes), -1, 4), e_r.reshape(len(boxes), -1, 4)
    wt = post.WEIGHTS
    assert (rel[..., 2:] / 5 < post.XFORM_CLIP - 1).all()          # the clamp of the size deltas is far
    pw, ph = np.exp(rel[..., 2] / wt[2]) * w[:, None], np.exp(rel[..., 3] / wt[3]) * h[:, None]
    pcx, pcy = rel[..., 0] / wt[0] * w[:, None] + cx[:, None], rel[..., 1] / wt[1] * h[:, None] + cy[:, None]
    dx = e_rel[..., 0] / wt[0] * w[:, None] + 0.5 * pw * np.expm1(e_rel[..., 2] / wt[2])
    dy = e_rel[..., 1] / wt[1] * h[:, None] + 0.5 * ph * np.expm1(e_rel[..., 3] / wt[3])
    corners = np.stack([pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph], -1)
    delta = np.maximum(dx, dy) + 8 * 2.0 ** -24 * np.maximum(np.abs(corners).max(-1), np.maximum(pw, ph))
    for b in range(2):
        rows = np.flatnonzero(im == b)
        net_h, net_w = NETS[b]
        bx = corners[rows].copy()
        bx[..., 0::2], bx[..., 1::2] = bx[..., 0::2].clip(0, net_w), bx[..., 1::2].clip(0, net_h)
        cand = []
        for r_, r in enumerate(rows):
            for k in range(1, case.K):
                note('score threshold', abs(sc[r, k] - SCORE_TH) / d_sc[r, k])
                if sc[r, k] > SCORE_TH:
                    side = min(bx[r_, k, 2] - bx[r_, k, 0], bx[r_, k, 3] - bx[r_, k, 1])
                    note('small box', abs(side - post.MIN_SIZE) / (2 * delta[r, k]))
                    if side >= post.MIN_SIZE:
                        cand.append((k, bx[r_, k], delta[r, k], sc[r, k], d_sc[r, k]))
        for p in range(len(cand)):
            for q in range(p):
                if cand[p][0] != cand[q][0]:
                    continue
                t = max(cand[p][2], cand[q][2])
                iou, move = iou_move(cand[p][1], cand[q][1], 100 * t)       # the bound of corners moved by 100 x their bound ...
                note('box nms iou', 101.0 if abs(iou - NMS_TH) > move else 100 * abs(iou - NMS_TH) / move)   # ... must not reach the threshold
                if iou + move > NMS_TH:
                    note('box nms order', abs(cand[p][3] - cand[q][3]) / (cand[p][4] + cand[q][4]))
    rpn_np = lambda f: (obj, dl)
    box_np = lambda r: (v_c.astype(F32), v_r.astype(F32))
    mask_layers = ref.mask_layers(sd)
    state = {}

    def mask_np(roi14):                                            # called once by the twin chain, on the final detections
        state['roi'] = np.asarray(roi14, F32)
        return ref.chain(mask_layers, state['roi'], 'float32')[0].astype(F32)
    twin, props2, per_image = pre.chain(feats, rpn_np, box_np, mask_np, NETS, PAD, [FRAME] * 2, NAMES, output_masks=True,
                                        rpn_options=dict(sizes=SIZES, pre_nms_top_n=PRE, post_nms_top_n=POST),
                                        head_options=dict(detections_per_img=PER_IMG, score_thresh=SCORE_TH, nms_thresh=NMS_TH))
    for b in range(2):
        note('detections_per_img not reached', np.inf if len(per_image[b]['scores']) < PER_IMG else 0.0)
    # ---- masks
    D = len(twin['rows'])
    if D:
        first = np.cumsum([0] + [len(p['boxes']) for p in props])
        d_det = np.array([delta[first[b] + per_image[b]['proposal'][j], per_image[b]['labels'][j]] for b, j in twin['rows']])
        labels = np.array([per_image[b]['labels'][j] for b, j in twin['rows']], np.int64)
        fmax = max(float(np.abs(f).max()) for f in feats)
        err0 = np.broadcast_to((12 * fmax * max(scales) * d_det)[:, None, None, None], state['roi'].shape)
        v_m, e_m = ref.chain(mask_layers, state['roi'], 'float32', err0=err0)
        ratio = max(FRAME[0] / min(n[0] for n in NETS), FRAME[1] / min(n[1] for n in NETS))
        M = v_m.shape[-1]
        for d in range(D):
            bq = twin['bboxes'][d].astype(np.float64)
            half = (M + 2) / M * 0.5
            edges = [(bq[2] + bq[0]) / 2 - (bq[2] - bq[0]) * half, (bq[3] + bq[1]) / 2 - (bq[3] - bq[1]) * half,
                     (bq[2] + bq[0]) / 2 + (bq[2] - bq[0]) * half, (bq[3] + bq[1]) / 2 + (bq[3] - bq[1]) * half]
            move = 2.2 * (d_det[d] * ratio + 8 * 2.0 ** -24 * np.abs(bq).max())          # (1 + (M + 2) / M) / 2 * 2 corners, and the float32 roundings
            for t in edges:
                note('mask box truncation', abs(t - np.round(t)) / move)
        v64, inside = post.paste_values64(v_m.astype(F32), twin['bboxes'], labels, FRAME)
        d_v = 0.25 * np.array([e_m[d, labels[d]].max() for d in range(D)])[:, None, None]
        note('mask threshold', (np.abs(v64 - MASK_TH) / d_v)[inside].min())
        state['mask_pixels_on'] = int((v64 > MASK_TH)[inside].sum())
    return m, dict(detections=D, images=len(set(twin['batch_im_id'].tolist())), labels=len(set(twin['label'].tolist())),
                   mask_pixels_on=state.get('mask_pixels_on', 0))


def search(seeds=range(200)):
    """what chose SEED: the first seed whose every margin exceeds 100 and whose case is not empty"""
    for seed in seeds:
        m, info = margins(seed)
        ok = min(m.values()) > 100 and info['detections'] > 3 and info['images'] == 2 and info['labels'] == 2 and info['mask_pixels_on'] > 0
        print(seed, 'ok' if ok else '--', info, {k: round(v, 1) for k, v in m.items() if v < 1e6})
        if ok:
            return seed
