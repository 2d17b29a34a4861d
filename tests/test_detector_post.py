"""The detector's output side on the GPU (csrc/kernels_detpost.hip behind cosypose_amd/detector.py) against the torch-CPU twin
tests/detpost_ref.py, which test_detector_post_host.py holds against hand-derived vectors.

Keep lists, kept (image, proposal, label) triples, labels and image ids are compared for EQUALITY.  Boxes: within 4 float32 ulps of the
larger coordinate of the box along the axis (the two sides run the same rounded operations and differ in their exp only: DESIGN.md
section 21); the step to the frame is checked bit for bit.  Scores: within (C + 4 + 16) 2^-24 relative of the float64 softmax.  Masks:
equal on every pixel whose float64 value is not within 1e-5 of mask_th; at most 0.1 % of a mask's in-box pixels may be that close."""
import numpy as np
import pytest
import torch

import detpost_ref as ref
from cosypose_amd import batched_nms, detections_from_heads, nms, paste_masks, postprocess_detections
from cosypose_amd import detector
from cosypose_amd.io_formats import make_detections

pytestmark = pytest.mark.gpu

NET, FRAME = (37, 53), (24, 40)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- NMS ---------------------------------------------------------------------------------------------------------------------------
def nms_case(N, seed=0):
    """integer boxes (every IoU exact), scores from a set of 16 values (equal scores), pairs at exactly IoU 1/2, labels 0 .. 2"""
    rng = np.random.RandomState(seed + N)
    x1, y1 = rng.randint(0, 40, N), rng.randint(0, 40, N)
    boxes = np.stack([x1, y1, x1 + rng.randint(1, 21, N), y1 + rng.randint(1, 21, N)], 1).astype(np.float32)
    if N >= 2:
        boxes[0], boxes[1] = [0, 0, 10, 10], [0, 0, 10, 5]                    # IoU 50 / 100: not suppressed at 0.5
    if N >= 65:
        boxes[63], boxes[64] = [30, 30, 50, 40], [30, 30, 50, 35]             # the same across a tile edge
    scores = (rng.randint(1, 17, N) / 16).astype(np.float32)
    labels = rng.randint(0, 3, N).astype(np.int64)
    return boxes, scores, labels


@pytest.mark.parametrize('N', [0, 1, 2, 63, 64, 65, 130])
def test_nms_and_batched_nms_equal_the_twin(N):
    boxes, scores, labels = nms_case(N)
    got = nms(dev(boxes), dev(scores), 0.5)
    assert got.dtype == torch.int64 and got.is_cuda
    want = ref.nms(boxes, scores, 0.5)
    assert got.cpu().tolist() == want.tolist()
    if N >= 63:
        assert 0 < len(want) < N and len(np.unique(scores[want])) < len(want)      # something suppressed; equal scores among the kept
    got_b = batched_nms(dev(boxes), dev(scores), dev(labels), 0.5)
    want_b = ref.batched_nms(boxes, scores, labels, 0.5)
    assert got_b.cpu().tolist() == want_b.tolist()
    assert batched_nms(dev(boxes), dev(scores), dev(labels.astype(np.int32)), 0.5).cpu().tolist() == want_b.tolist()
    if N >= 63:
        assert len(want_b) > len(want)                                              # the shift matters


def test_nms_exact_threshold_and_ties():
    boxes = np.array([[0, 0, 10, 10], [0, 0, 10, 5], [0, 0, 10, 6], [5, 0, 15, 10]], np.float32)      # IoU with box 0: 1/2, 6/10, 1/3
    scores = np.array([.9, .8, .7, .6], np.float32)
    assert nms(dev(boxes), dev(scores), 0.5).cpu().tolist() == [0, 1, 3]
    assert nms(dev(boxes), dev(scores), 0.49).cpu().tolist() == [0, 3]
    same = np.array([[0, 0, 10, 10], [0, 0, 10, 10], [20, 20, 30, 30]], np.float32)
    assert nms(dev(same), dev(np.full(3, .5, np.float32)), 0.5).cpu().tolist() == [0, 2]
    assert batched_nms(dev(same), dev(np.array([.9, .8, .7], np.float32)), dev(np.array([1, 2, 1])), 0.5).cpu().tolist() == [0, 1, 2]
    assert batched_nms(dev(same[[0, 0, 0]]), dev(np.array([.9, .8, .7], np.float32)), dev(np.array([1, 2, 1])), 0.5).cpu().tolist() == [0, 1]


def test_nms_chain_across_a_block_boundary():
    # scores fall with the index, so row = index.  Box 70 overlaps box 3 only; 3 overlaps 2, but 2 is suppressed by 1: 3 survives and
    # suppresses 70 through the (row block 0, column block 1) tile
    N = 130
    boxes = np.array([[100 * i, 0, 100 * i + 10, 10] for i in range(N)], np.float32)
    boxes[1], boxes[2], boxes[3] = [20000, 0, 20010, 10], [20000, 0, 20010, 8], [20000, 6, 20010, 20]
    boxes[70] = [20000, 6, 20010, 18]
    scores = (1 - np.arange(N) / 256).astype(np.float32)
    want = ref.nms(boxes, scores, 0.5)
    assert 1 in want and 2 not in want and 3 in want and 70 not in want and len(want) == N - 2
    assert nms(dev(boxes), dev(scores), 0.5).cpu().tolist() == want.tolist()


def test_nms_three_images_in_one_call_the_middle_one_empty():
    (b0, s0, l0), (b2, s2, l2) = nms_case(65, 1), nms_case(130, 2)
    boxes, scores, labels = np.concatenate([b0, b2]), np.concatenate([s0, s2]), np.concatenate([l0, l2])
    order = np.concatenate([np.array(ref.visiting_order(s0)), 65 + np.array(ref.visiting_order(s2))]).astype(np.int64)
    max_coord = np.array([b0.max(), 0, b2.max()], np.float32)
    seg_start, seg_count = np.array([0, 65, 65], np.int32), np.array([65, 0, 130], np.int32)
    kept, n_kept, flags = detector._nms_segments(dev(boxes), dev(order), dev(labels.astype(np.int32)), dev(max_coord), dev(seg_start),
                                                 dev(seg_count), 3, 192, 0.5, 40, flags=True)
    kept, n_kept, flags = kept.cpu().numpy(), n_kept.cpu().numpy(), flags.cpu().numpy()
    want0, want2 = ref.batched_nms(b0, s0, l0, 0.5, 40), 65 + ref.batched_nms(b2, s2, l2, 0.5, 40)
    assert n_kept.tolist() == [len(want0), 0, len(want2)] and len(want2) == 40          # the cut is exercised in image 2
    assert kept[0, :n_kept[0]].tolist() == want0.tolist() and kept[2, :n_kept[2]].tolist() == want2.tolist()
    assert (kept[1] == -1).all() and (kept[0, n_kept[0]:] == -1).all()
    assert np.flatnonzero(flags).tolist() == sorted(want0.tolist() + want2.tolist())


# ---- heads -> boxes ----------------------------------------------------------------------------------------------------------------
def ulps(got, want):
    """|got - want| in float32 ulps of the larger coordinate of the box along the axis"""
    got, want = np.asarray(got, np.float32).reshape(-1, 2, 2), np.asarray(want, np.float32).reshape(-1, 2, 2)
    mag = np.abs(want).max(1, keepdims=True)
    return np.abs(got.astype(np.float64) - want) / np.spacing(np.maximum(mag, np.float32(1e-30)))


@pytest.mark.parametrize('R', [1, 70])
@pytest.mark.parametrize('C', [2, 5])
def test_postprocess_detections_equals_the_twin(R, C):
    logits, reg, props = ref.head_case(100 + R + C, [R, R], C, NET)
    s64 = ref.scores64(logits)
    assert int(((s64[:, 1:] - 0.05).abs() < 1e-4).sum()) == 0                          # no score too close to the threshold to call
    if R >= 2:
        assert 0.05 < float(s64[1, 1]) < 0.05 + 1e-3
    want = ref.postprocess(logits, reg, props, [NET] * 2, [FRAME] * 2, detections_per_img=3)
    uncut = ref.postprocess(logits, reg, props, [NET] * 2, [FRAME] * 2, detections_per_img=1000)
    if R == 70:
        assert all(len(u['scores']) > 3 for u in uncut)                                  # the cut to 3 is exercised
        assert (1, 1) in set(zip(uncut[0]['proposal'].tolist(), uncut[0]['labels'].tolist()))      # the near-threshold candidate survives
    args = (dev(logits), dev(reg), [dev(p) for p in props], [NET] * 2)
    boxes, scores, labels, im_ids, src = postprocess_detections(*args, original_sizes=[FRAME] * 2, detections_per_img=3, return_source=True)
    boxes_net = postprocess_detections(*args, detections_per_img=3)[0]
    assert boxes.dtype == torch.float32 and scores.dtype == torch.float32 and labels.dtype == torch.int64 and im_ids.dtype == torch.int64
    w_im = np.concatenate([np.full(len(o['scores']), b) for b, o in enumerate(want)])
    w_prop, w_label = np.concatenate([o['proposal'] for o in want]), np.concatenate([o['labels'] for o in want])
    assert im_ids.cpu().tolist() == w_im.tolist() and labels.cpu().tolist() == w_label.tolist()
    assert (src.cpu().numpy() // (C - 1)).tolist() == w_prop.tolist() and (src.cpu().numpy() % (C - 1) + 1).tolist() == w_label.tolist()
    first = np.array([0, R])[w_im]
    err_s = np.abs(scores.cpu().numpy().astype(np.float64) / s64.numpy()[first + w_prop, w_label] - 1)
    err_b = ulps(boxes_net.cpu().numpy(), np.concatenate([o['boxes_net'] for o in want]))
    print(f'R={R} C={C}: D={len(w_im)} score err {err_s.max():.3g} (bound {(C + 20) * 2.0 ** -24:.3g}), box err {err_b.max():.3g} ulps (bound 4)')
    assert err_s.max() <= (C + 4 + 16) * 2.0 ** -24
    assert err_b.max() <= 4
    ratio = np.array([np.float32(FRAME[1]) / np.float32(NET[1]), np.float32(FRAME[0]) / np.float32(NET[0])] * 2, np.float32)
    assert np.array_equal(boxes.cpu().numpy(), boxes_net.cpu().numpy() * ratio)         # step 6: one multiplication, bit for bit
    one = postprocess_detections(dev(logits), dev(reg), dev(np.concatenate(props)), [NET] * 2, [FRAME] * 2, detections_per_img=3, counts=[R, R])
    assert torch.equal(one[0], boxes) and torch.equal(one[1], scores)


def test_postprocess_refuses_more_candidates_than_the_cap():
    logits, reg, props = ref.head_case(7, [70, 70], 5, NET)
    n = [int((ref.scores32(logits[i * 70:(i + 1) * 70])[:, 1:] > 0.05).sum()) for i in range(2)]
    assert max(n) > 64
    with pytest.raises(ValueError, match='more than max_candidates = 64'):
        postprocess_detections(dev(logits), dev(reg), [dev(p) for p in props], [NET] * 2, max_candidates=64)


# ---- masks -------------------------------------------------------------------------------------------------------------------------
PASTE_BOXES = np.array([[10.3, 8.2, 30.7, 25.9],                  # inside
                        [-5.5, 10, 8, 20], [20, -6.2, 35, 7.5], [45, 12, 60.4, 30], [12, 30, 28, 44.3],      # across each edge
                        [70, 50, 90, 60], [-30, -30, -10, -5],    # wholly outside
                        [3.2, 4.1, 3.4, 4.3],                     # one pixel
                        [-20, -15, 80, 60]], np.float32)          # larger than the frame


@pytest.mark.parametrize('frame', [(37, 53), (24, 40), (130, 128)])      # scalar stores; 16-byte stores that cross rows; two workgroups of them
@pytest.mark.parametrize('M', [14, 28])
@pytest.mark.parametrize('mask_th', [0.5, 0.8])
def test_paste_masks_equals_the_twin(M, mask_th, frame):
    H, W = frame
    boxes = PASTE_BOXES * np.array([W / 53, H / 37, W / 53, H / 37], np.float32)
    boxes[7] = PASTE_BOXES[7]
    D, C = len(boxes), 3
    logits = ref.smooth_mask_logits(M, D, C, M)
    labels = np.arange(D) % C
    v64, inside = ref.paste_values(logits, boxes, labels, frame, torch.float64)
    want = ref.paste_masks(logits, boxes, labels, frame, mask_th)
    close = ((v64 - mask_th).abs() <= 1e-5).numpy() & inside.numpy()
    in_box = inside.numpy().reshape(D, -1).sum(1)
    assert (close.reshape(D, -1).sum(1) <= 1e-3 * in_box).all()                         # the twin alone stays inside the exclusion cap
    assert in_box[5] == 0 and in_box[6] == 0 and in_box[7] == 1 and in_box[8] == H * W
    out = torch.ones((D, H, W), dtype=torch.bool, device='cuda')                        # every pixel must be written
    got = paste_masks(dev(logits), dev(boxes), dev(labels), frame, mask_th, out=out)
    assert got is out and got.dtype == torch.bool
    got = got.view(torch.uint8).cpu().numpy()
    assert set(np.unique(got)) <= {0, 1}
    differ = (got.astype(bool) != want) & ~close
    assert differ.sum() == 0, np.argwhere(differ)[:10]
    assert not got[5].any() and not got[6].any() and want[0].any() and want[8].any() and got[7].sum() == 1
    fresh = paste_masks(dev(logits), dev(boxes), dev(labels.astype(np.int32)), frame, mask_th)
    assert torch.equal(fresh, out)
    bad = paste_masks(dev(logits), dev(boxes), dev(np.full(D, C)), frame, mask_th)      # a label outside the channels: empty masks
    assert not bad.any()


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def e2e_case():
    C, M = 4, 14
    logits, reg, props = ref.head_case(16, [40, 25], C, NET)
    logits = (logits * 0.25).astype(np.float32)                    # flatter softmaxes: scores on both sides of detection_th = 0.3
    per_image = ref.postprocess(logits, reg, props, [NET] * 2, [FRAME] * 2, detections_per_img=100)
    s64 = ref.scores64(logits)[:, 1:]
    assert int(((s64 - 0.05).abs() < 1e-4).sum()) == 0 and int(((s64 - 0.3).abs() < 1e-4).sum()) == 0       # nothing too close to a threshold
    kept = np.sort(np.concatenate([o['scores'] for o in per_image]).astype(np.float64))
    assert (np.diff(kept) > 4e-6 * kept[1:]).all()                 # ... or to another score: the ranking is not a matter of rounding
    assert len(kept) > (kept > 0.3).sum() > 0
    names = {c: f'obj_{c:06d}' for c in range(1, C)}
    mask_logits = [ref.smooth_mask_logits(11 + b, len(out['scores']), C, M) for b, out in enumerate(per_image)]
    return C, M, logits, reg, props, per_image, names, mask_logits


E2E = {}


@pytest.mark.parametrize('detection_th', [None, 0.3])
@pytest.mark.parametrize('one_instance_per_class', [False, True])
@pytest.mark.parametrize('output_masks', [False, True])
def test_detections_from_heads_equals_make_detections_on_the_twin(detection_th, one_instance_per_class, output_masks):
    if not E2E:
        E2E['case'] = e2e_case()
    C, M, logits, reg, props, per_image, names, mask_logits = E2E['case']
    net_rows = np.concatenate([o['boxes_net'] for o in per_image])
    row_im = np.concatenate([np.full(len(o['scores']), b) for b, o in enumerate(per_image)])
    all_logits = np.concatenate(mask_logits)
    calls = []

    def mask_head(boxes_net, batch_im_id):
        assert boxes_net.is_cuda and batch_im_id.is_cuda and batch_im_id.dtype == torch.int64
        bn, bi = boxes_net.cpu().numpy(), batch_im_id.cpu().numpy()
        rows = [int(np.argmin(np.abs(net_rows - x).max(1) + 1e6 * (row_im != b))) for x, b in zip(bn, bi)]
        calls.append((bn, bi, rows))
        return dev(all_logits[rows])
    got = detections_from_heads(dev(logits), dev(reg), [dev(p) for p in props], [NET] * 2, [FRAME] * 2, names, mask_head=mask_head,
                                detection_th=detection_th, one_instance_per_class=one_instance_per_class, output_masks=output_masks,
                                detections_per_img=100)
    fed = [dict(boxes=out['boxes'], labels=[names[int(l)] for l in out['labels']], scores=out['scores'],
                masks=ref.paste_values(mask_logits[b], out['boxes'], out['labels'], FRAME)[0][:, None]) for b, out in enumerate(per_image)]
    want = make_detections(fed, device='cuda', detection_th=detection_th, one_instance_per_class=one_instance_per_class,
                           output_masks=output_masks, mask_th=0.8)
    twin = ref.get_detections(per_image, names, None, FRAME, detection_th, one_instance_per_class)
    assert len(want.infos) > 0 and list(got.infos.columns) == list(want.infos.columns)
    assert got.infos['batch_im_id'].tolist() == want.infos['batch_im_id'].tolist() and got.infos['label'].tolist() == want.infos['label'].tolist()
    assert got.infos['score'].dtype == want.infos['score'].dtype
    assert np.abs(got.infos['score'].values / want.infos['score'].values - 1).max() <= (C + 4 + 16) * 2.0 ** -24 * 2    # both sides are float32 softmaxes
    assert got.bboxes.is_cuda and got.bboxes.dtype == torch.float32
    assert ulps(got.bboxes.cpu().numpy(), want.bboxes.cpu().numpy()).max() <= 5         # 4 of the decode and the rounding of step 6
    assert hasattr(got, 'masks') == output_masks == (len(calls) == 1)
    if output_masks:
        bn, bi, rows = calls[0]
        want_rows = [int(np.flatnonzero(row_im == b)[0]) + j for b, j in twin['rows']]
        assert rows == want_rows and bi.tolist() == twin['batch_im_id'].tolist()        # called once, with the twin's boxes, filters applied
        assert ulps(bn, net_rows[want_rows]).max() <= 4
        v64 = torch.cat([ref.paste_values(mask_logits[b], o['boxes'], o['labels'], FRAME, torch.float64)[0] for b, o in enumerate(per_image)])
        assert int(((v64 - 0.8).abs() <= 1e-5).sum()) == 0                              # no pixel too close to call: the masks must be equal
        assert got.masks.dtype == torch.bool and tuple(got.masks.shape) == (len(want_rows),) + FRAME
        assert torch.equal(got.masks, want.masks) and bool(want.masks.any())
        again = detections_from_heads(dev(logits), dev(reg), [dev(p) for p in props], [NET] * 2, [FRAME] * 2, names, mask_logits=dev(all_logits),
                                      detection_th=detection_th, one_instance_per_class=one_instance_per_class, output_masks=True,
                                      detections_per_img=100)
        assert torch.equal(again.masks, got.masks) and torch.equal(again.bboxes, got.bboxes)


def test_detections_from_heads_with_nothing_found():
    logits = np.full((9, 3), -8, np.float32)
    logits[:, 0] = 8
    _, reg, props = ref.head_case(1, [4, 5], 3, NET)

    def mask_head(boxes_net, batch_im_id):
        raise AssertionError('no detection, no mask head')
    got = detections_from_heads(dev(logits), dev(reg), [dev(p) for p in props], [NET] * 2, [FRAME] * 2, {1: 'a', 2: 'b'}, mask_head=mask_head,
                                output_masks=True)
    want = make_detections([dict(boxes=np.zeros((0, 4), np.float32), labels=[], scores=np.zeros(0, np.float32))] * 2, device='cuda',
                           output_masks=True)
    assert len(got.infos) == 0 and list(got.infos.columns) == list(want.infos.columns)
    assert tuple(got.bboxes.shape) == (0, 4) and got.bboxes.dtype == want.bboxes.dtype and got.bboxes.is_cuda
    assert not hasattr(got, 'masks') and not hasattr(want, 'masks')
    boxes, scores, labels, im_ids = postprocess_detections(dev(logits), dev(reg), [dev(p) for p in props], [NET] * 2)
    assert tuple(boxes.shape) == (0, 4) and len(scores) == len(labels) == len(im_ids) == 0
