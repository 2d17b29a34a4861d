"""The detector's training side on the GPU (csrc/kernels_dettrain.hip behind cosypose_amd/detector_train.py) against the CPU twin
tests/dettrain_ref.py, which test_detector_train_host.py holds against hand-derived vectors.

Match indices, labels, sampled sets and counts are compared for EQUALITY; mask targets BIT for bit with the float32 twin; encodes, losses and
gradients against the twin's float64 evaluation of the same float32 inputs within the bounds the twin derives beside them (section 23: built from
the operation count and the ulp errors of expf, logf and log1pf, never from what the kernels give).  Every test prints the measured share of its
bound before it asserts."""
import ctypes

import numpy as np
import pytest
import torch

import detpre_ref as pre
import dettrain_ref as ref
from cosypose_amd import _lib, detector_train as dt

pytestmark = pytest.mark.gpu
f32 = np.float32
U = ref.U

GRID, A = [(5, 7), (3, 4), (1, 2)], 3                               # section 22's grid: 105 + 36 + 6 anchors per image
SIZES, RATIOS = ((32,), (64,), (128,)), (0.5, 1.0, 2.0)
PAD, NETS, FRAME = (40, 56), [(37, 53), (40, 50)], (24, 40)
ANCHORS = pre.anchors(GRID, PAD, SIZES, RATIOS)
N_ANCHORS = len(ANCHORS)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def share(name, err, bound):
    """print the largest error as a share of its bound, then hold it"""
    err, bound = np.broadcast_arrays(np.asarray(err, np.float64), np.asarray(bound, np.float64))
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f'{name}: largest error / bound = {worst:.3f} (bound: 1)')
    assert np.isfinite(err).all() and (err <= bound).all(), (name, worst)


def random_boxes(rng, n, h=PAD[0], w=PAD[1], low=2.0):
    x1, y1 = rng.uniform(-8, w - 8, n), rng.uniform(-8, h - 8, n)
    return np.stack([x1, y1, x1 + rng.uniform(low, w, n), y1 + rng.uniform(low, h, n)], 1).astype(f32)


# ---- match ---------------------------------------------------------------------------------------------------------------------------
def check_match(gt, candidates, high, low, lq, counts=None, gt_labels=None):
    """candidates: None (the anchor grid) or (B,N,4); -> the device's matched (B,N), iou (B,N) after equality with the twin"""
    B = len(gt)
    grid = dt.AnchorGrid(GRID, PAD, SIZES, RATIOS) if candidates is None else None
    out = dt.match_boxes([dev(g) for g in gt], grid if candidates is None else dev(candidates), high, low, lq,
                         counts=None if counts is None else dev(np.asarray(counts, np.int32)),
                         gt_labels=None if gt_labels is None else [dev(np.asarray(l, np.int64)) for l in gt_labels])
    matched, iou = host(out[0]), host(out[1])
    for b in range(B):
        cand = ANCHORS if candidates is None else candidates[b]
        m, v = ref.match(gt[b], cand, high, low, lq, None if counts is None else counts[b])
        assert np.array_equal(matched[b], m), (b, np.flatnonzero(matched[b] != m)[:8])
        assert np.array_equal(iou[b].view(np.uint32), v.view(np.uint32))
        if gt_labels is not None:
            assert np.array_equal(host(out[2])[b], ref.labels_of(m, gt_labels[b]))
    return matched, iou


@pytest.mark.parametrize('G', [1, 3, 65])                              # 65: more than a wave of ground truths
def test_match_equals_the_twin(G):
    rng = np.random.RandomState(G)
    gt = [random_boxes(rng, G), random_boxes(rng, 2)]
    for lq in (False, True):
        matched, iou = check_match(gt, None, 0.7, 0.3, lq)
        # each image alone: bit-equal to its rows in the batch
        for b in range(2):
            alone = dt.match_boxes([dev(gt[b])], dt.AnchorGrid(GRID, PAD, SIZES, RATIOS), 0.7, 0.3, lq)
            assert np.array_equal(host(alone[0])[0], matched[b]) and np.array_equal(host(alone[1])[0].view(np.uint32), iou[b].view(np.uint32))
    if G == 65:                                                           # the restore does something, and to an anchor that is "between"
        plain, restored = ref.match(gt[0], ANCHORS, 0.7, 0.3, False)[0], ref.match(gt[0], ANCHORS, 0.7, 0.3, True)[0]
        assert ((plain == -2) & (restored >= 0)).any() and ((plain == -1) & (restored >= 0)).any()


def test_match_special_ground_truths():
    k = (2 * 7 + 3) * A + 1                                               # level 0, cell (2, 3), a = 1: [8, 0, 40, 32]
    assert ANCHORS[k].tolist() == [8, 0, 40, 32]
    gt = [np.array([ANCHORS[k], [4, 4, 30, 20], [4, 4, 30, 20], [12, 9, 12, 30], [9, 9, 9, 9]], f32),       # an anchor, two identical, zero areas
          np.array([[10, 5, 44, 30], [900, 900, 950, 950]], f32)]                                             # one outside every anchor
    for lq in (False, True):
        matched, iou = check_match(gt, None, 0.7, 0.3, lq, gt_labels=[[5, 6, 7, 8, 9], [3, 4]])
        assert matched[0][k] == 0 and iou[0][k] == 1.0
        assert not (matched[0] == 2).any() and (matched[0] == 1).any() == lq   # identical ground truths: the lower index wins (0.7 is reached by none)
    # best[g] == 0 (torchvision's behaviour, kept): the ground truth outside restores EVERY anchor, each to its own argmax
    assert (matched[1] >= 0).all() and (iou[1] < 0.3).any()
    assert (ref.match(gt[1], ANCHORS, 0.7, 0.3, False)[0] == -1).any()
    # "between" for its best ground truth and the best anchor of another one: the hand case of the host test, on the boxes path
    hand_gt, hand_c = np.array([[0, 0, 10, 10], [0, 3, 10, 5]], f32), np.array([[[0, 0, 10, 10], [0, 0, 10, 5]]], f32)
    assert check_match([hand_gt], hand_c, 0.7, 0.3, False)[0].tolist() == [[0, -2]]
    assert check_match([hand_gt], hand_c, 0.7, 0.3, True)[0].tolist() == [[0, 0]]


def test_match_thresholds_on_both_sides_of_an_iou():
    rng = np.random.RandomState(7)
    gt = [random_boxes(rng, 3)]
    iou = ref.box_iou(gt[0], ANCHORS)
    val, arg = iou.max(0), iou.argmax(0)
    j = int(np.argmin(np.abs(val - 0.45)))                                # an anchor whose best IoU is an ordinary float32 between 0 and 1
    v = val[j]
    up = np.nextafter(v, f32(1))
    assert 0 < v < 1 and up > v
    got = [check_match(gt, None, high, low, False)[0][0][j] for high, low in ((v, v), (up, v), (up, up))]
    assert got == [arg[j], -2, -1]                                        # val < high and val < low are strict


def test_match_best_crosses_workgroups():
    grid_sizes, pad = [(153, 153)], (612, 612)                           # 70 227 anchors in one level: 275 workgroups per image
    anchors = pre.anchors(grid_sizes, pad, ((32,),), RATIOS)
    gt = np.array([[100, 100, 140, 160], [300.5, 20.25, 340, 50], [5, 500, 600, 610]], f32)
    grid = dt.AnchorGrid(grid_sizes, pad, ((32,),), RATIOS)
    assert grid.N == len(anchors) == 70227
    out = dt.match_boxes([dev(gt)], grid, 0.7, 0.3, True)
    m, v = ref.match(gt, anchors, 0.7, 0.3, True)
    assert np.array_equal(host(out[0])[0], m) and np.array_equal(host(out[1])[0].view(np.uint32), v.view(np.uint32))
    assert (m == 2).any() and ref.match(gt, anchors, 0.7, 0.3, False)[0].max() < 2      # the wide ground truth is matched through the restore alone


def test_match_boxes_path_with_padded_rows():
    rng = np.random.RandomState(11)
    gt = [random_boxes(rng, 3), random_boxes(rng, 5)]
    cand = np.stack([random_boxes(rng, 300), random_boxes(rng, 300)])
    cand[0, 7] = 0                                                       # a zero row among the real ones
    cand[0, :3] = gt[0]
    for lq in (False, True):
        matched, _ = check_match(gt, cand, 0.5, 0.5, lq, counts=[298, 3], gt_labels=[[1, 2, 3], [4, 5, 6, 7, 8]])
        assert (matched[0][298:] == -3).all() and (matched[1][3:] == -3).all() and matched[0][7] == -1
        assert matched[0][:3].tolist() == [0, 1, 2]


# ---- sampler -------------------------------------------------------------------------------------------------------------------------
PN = [(P, N) for P in (0, 1, 127, 128, 129, 400) for N in (0, 5, 1000)]


def sampler_labels(rng, n=1500):
    labels = np.full((len(PN), n), -1, np.int32)
    for b, (P, N) in enumerate(PN):
        at = rng.permutation(n)
        labels[b, at[:P]] = rng.randint(1, 6, P)
        labels[b, at[P:P + N]] = 0
    return labels


@pytest.mark.parametrize('bs,frac', [(256, 0.5), (512, 0.25), (4, 0.5)])
@pytest.mark.parametrize('kind', ['nine', 'equal', 'random'])
def test_sampler_equals_the_twin(bs, frac, kind):
    rng = np.random.RandomState(bs)
    labels = sampler_labels(rng)
    B, n = labels.shape
    keys = dict(nine=rng.randint(0, 9, (B, n)) * 1000003, equal=np.full((B, n), 77), random=rng.randint(0, 2 ** 31 - 1, (B, n)))[kind].astype(np.int32)
    samp_idx, samp_count, pos_idx, pos_count = (host(t) for t in dt.sample_balanced(dev(labels), bs, frac, keys=dev(keys)))
    assert samp_idx.shape == (B, bs) and pos_idx.shape == (B, int(bs * frac))
    for b, (P, N) in enumerate(PN):
        samp, pos = ref.sample(labels[b], keys[b], bs, frac)
        n_pos = min(int(bs * frac), P)
        assert (len(pos), len(samp)) == (n_pos, n_pos + min(bs - n_pos, N)) == (pos_count[b], samp_count[b])
        assert samp_idx[b, :len(samp)].tolist() == samp.tolist() and (samp_idx[b, len(samp):] == -1).all()
        assert pos_idx[b, :len(pos)].tolist() == pos.tolist() and (pos_idx[b, len(pos):] == -1).all()


def test_sampler_draws_its_own_keys():
    labels = dev(sampler_labels(np.random.RandomState(0)))
    g = torch.Generator(device='cuda').manual_seed(5)
    a = dt.sample_balanced(labels, 256, 0.5, generator=g)
    b = dt.sample_balanced(labels, 256, 0.5, generator=torch.Generator(device='cuda').manual_seed(5))
    c = dt.sample_balanced(labels, 256, 0.5, generator=torch.Generator(device='cuda').manual_seed(6))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[0], c[0])
    lab = host(labels)
    for row, idx, cnt in zip(lab, host(a[0]), host(a[1])):
        assert (row[idx[:cnt]] >= 0).all() and (np.diff(idx[:cnt]) > 0).all()


# ---- encode --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('weights', [ref.RPN_WEIGHTS, ref.ROI_WEIGHTS])
def test_encode_against_float64(weights):
    rng = np.random.RandomState(2)
    prop, gt = random_boxes(rng, 300), random_boxes(rng, 300)
    prop[5, 2] = prop[5, 0]                                              # a zero-width proposal: inf, and 0 / 0 for an equal centre
    prop[6] = [3, 4, 3, 9]; gt[6] = [1, 4, 5, 9]
    gt[7, 3] = gt[7, 1]                                                  # a zero-height ground truth: log(0) = -inf
    got = host(dt.encode_boxes(dev(gt), dev(prop), weights)).astype(np.float64)
    with np.errstate(all='ignore'):
        twin = ref.encode(gt, prop, weights)
        want, bound = ref.encode(gt, prop, weights, np.float64)
    odd = ~np.isfinite(want)
    assert odd[5, 0] and odd[5, 2] and odd[6, 0] and odd[7, 3] and odd.sum() == 5
    assert np.array_equal(np.isnan(got), np.isnan(twin)) and np.array_equal(np.isinf(got), np.isinf(twin))
    assert np.array_equal(got[odd & ~np.isnan(twin)], twin[odd & ~np.isnan(twin)].astype(np.float64))
    share(f'encode {weights}', np.abs(got[~odd] - want[~odd]), bound[~odd])


# ---- RPN loss ------------------------------------------------------------------------------------------------------------------------
def rpn_case(seed):
    rng = np.random.RandomState(seed)
    obj = [rng.normal(0, 2, (2, A, H, W)).astype(f32) for H, W in GRID]
    dl = [rng.normal(0, 0.5, (2, 4 * A, H, W)).astype(f32) for H, W in GRID]
    special = np.array([0, 100, -100, 1e4, -1e4], f32)
    for o in obj:
        flat = o.reshape(-1)
        flat[rng.permutation(flat.size)[:flat.size // 3]] = special[rng.randint(0, 5, flat.size // 3)]
    gt = [np.array([[8, 0, 40, 32], [20, 10, 50, 38], [0, 0, 20, 18]], f32), np.array([[2, 3, 30, 30], [25, 5, 55, 35]], f32)]
    keys = rng.randint(0, 2 ** 31 - 1, (2, N_ANCHORS)).astype(np.int32)
    return obj, dl, gt, keys


def targets_of(gt, labels=None, masks=None):
    return [dict(boxes=dev(g), labels=dev(np.asarray(labels[b] if labels else np.ones(len(g)), np.int64)),
                 masks=dev(masks[b]) if masks else torch.zeros((len(g),) + FRAME, dtype=torch.uint8, device='cuda')) for b, g in enumerate(gt)]


@pytest.mark.parametrize('bs', [256, 16])                              # everything that is not ignored, and a real subsample
def test_rpn_loss_and_gradients(bs):
    obj, dl, gt, keys = rpn_case(bs)
    want = ref.rpn_loss(obj, dl, gt, PAD, SIZES, RATIOS, keys, bs)
    n_s = want['n_sampled']
    assert n_s > 8 and any((want['matched'][b][s] >= 0).any() for b, s in enumerate(want['sampled']))

    def run():
        o, d = [dev(t).requires_grad_() for t in obj], [dev(t).requires_grad_() for t in dl]
        l_obj, l_box, (matched, samp_idx, samp_count) = dt.rpn_loss(o, d, targets_of(gt), NETS, PAD, SIZES, RATIOS, keys=dev(keys), batch_size_per_image=bs,
                                                                    return_samples=True)
        (2 * l_obj + 3 * l_box).backward()
        return l_obj, l_box, matched, samp_idx, samp_count, [t.grad for t in o], [t.grad for t in d]
    l_obj, l_box, matched, samp_idx, samp_count, g_obj, g_dl = run()
    assert np.array_equal(host(matched), want['matched'])
    for b, s in enumerate(want['sampled']):
        assert host(samp_count)[b] == len(s) and host(samp_idx)[b, :len(s)].tolist() == s.tolist()
    for name, got in (('loss_objectness', l_obj), ('loss_rpn_box_reg', l_box)):
        share(f'{name} (bs {bs})', abs(got.item() - want['losses'][name]), want['bounds'][name])
    for l in range(len(GRID)):
        go, gd = host(g_obj[l]).astype(np.float64) / 2, host(g_dl[l]).astype(np.float64) / 3
        assert np.isfinite(go).all() and np.isfinite(gd).all()
        assert not go[want['grad_objectness'][l] == 0].any() and not gd[want['grad_deltas'][l] == 0].any()      # not sampled: exactly 0
        share(f'grad objectness level {l}', np.abs(go - want['grad_objectness'][l]), (ref.SIGMOID_GRAD_BOUND + 2 * U) / n_s)
        share(f'grad deltas level {l}', np.abs(gd - want['grad_deltas'][l]), 3 * U / n_s)
    again = run()
    assert again[0].item() == l_obj.item() and again[1].item() == l_box.item()                                   # two calls: the same bits
    assert all(torch.equal(a, b) for a, b in zip(again[5] + again[6], g_obj + g_dl))


# ---- Fast R-CNN loss ---------------------------------------------------------------------------------------------------------------------
def frc_case(R, C, seed=0):
    rng = np.random.RandomState(seed + R + C)
    z = rng.normal(0, 3, (R, C)).astype(f32)
    z.reshape(-1)[rng.permutation(R * C)[:R * C // 4]] = np.array([0, 100, -100, 1e4, -1e4], f32)[rng.randint(0, 5, R * C // 4)]
    d, t = rng.normal(0, 1, (R, 4 * C)).astype(f32), rng.normal(0, 1, (R, 4)).astype(f32)
    labels = rng.randint(0, C, R)
    labels[rng.permutation(R)[:R // 3]] = 0
    if R > 4:
        labels[R // 2 - 1:R // 2 + 2] = -1                               # padding rows in the middle of a block
        # |d - t| exactly at beta = 1, and one float on either side of it
        labels[:3], t[:3, 0] = 1, 2
        d[:3, 4] = [3, np.nextafter(f32(3), f32(4)), np.nextafter(f32(3), f32(2))]
    return z, d, labels, t


@pytest.mark.parametrize('C', [2, 22, 91])
@pytest.mark.parametrize('R', [1, 65, 2 * 512])
def test_fastrcnn_loss_and_gradients(R, C):
    z, d, labels, t = frc_case(R, C)
    want = ref.fastrcnn_loss(z, d, labels, t)

    def run():
        zz, dd = dev(z).requires_grad_(), dev(d).requires_grad_()
        l_cls, l_box = dt.fastrcnn_loss(zz, dd, dev(labels.astype(np.int32)), dev(t))
        (2 * l_cls + 3 * l_box).backward()
        return l_cls, l_box, zz.grad, dd.grad
    l_cls, l_box, gz, gd = run()
    share(f'loss_classifier R {R} C {C}', abs(l_cls.item() - want['losses']['loss_classifier']), want['bounds']['loss_classifier'])
    share(f'loss_box_reg R {R} C {C}', abs(l_box.item() - want['losses']['loss_box_reg']), want['bounds']['loss_box_reg'])
    gz64, gd64 = host(gz).astype(np.float64) / 2, host(gd).astype(np.float64) / 3
    assert np.isfinite(gz64).all() and np.isfinite(gd64).all()
    assert not gz64[labels < 0].any() and not gd64[want['grad_box'] == 0].any()
    share('grad class_logits', np.abs(gz64 - want['grad_logits']), want['grad_logits_bound'] + 0 * gz64)
    share('grad box_regression', np.abs(gd64 - want['grad_box']), want['grad_box_bound'])
    again = run()
    assert again[0].item() == l_cls.item() and again[1].item() == l_box.item() and torch.equal(again[2], gz) and torch.equal(again[3], gd)


def test_fastrcnn_loss_of_an_all_background_batch():
    z, d, labels, t = frc_case(65, 22)
    labels = np.where(labels < 0, -1, 0)
    zz, dd = dev(z).requires_grad_(), dev(d).requires_grad_()
    l_cls, l_box = dt.fastrcnn_loss(zz, dd, dev(labels.astype(np.int32)), dev(t))
    (l_cls + l_box).backward()
    assert l_box.item() == 0.0 and not dd.grad.any() and l_cls.item() > 0 and zz.grad.any()


# ---- mask targets and loss ---------------------------------------------------------------------------------------------------------------
def mask_case(M):
    rng = np.random.RandomState(M)
    masks = (rng.uniform(0, 1, (3,) + FRAME) < 0.5).astype(np.uint8)
    masks[1, 6:18, 10:30] = 1
    boxes = np.array([[3.2, 4.1, 3.9, 20.3],                           # a side below 1
                      [2, 1, 2 + M, 15] if M <= 36 else [2, 1, 38, 1 + M],     # a side of exactly M: g = 1
                      [1, 0.5, 1.5 + M, 20] if M <= 36 else [1, 0.5, 30, 1 + M],  # a side of M + 0.5: g = 2
                      [0, 0, 40, 24],                                    # the whole frame
                      [5, 2, 39, 9],                                     # g_h != g_w
                      [30, 10, 70, 50],                                  # beyond the frame
                      [-10.5, -6.25, 12, 9],                             # negative coordinates
                      [-100, -50, 200, 100],                             # far larger than the frame
                      [0, 0, 0, 0],                                      # a zero row
                      [50, 30, 60, 40]], f32)                            # outside the frame altogether
    matched = np.array([0, 1, 2, 0, 1, 2, 0, 1, 2, 0], np.int32)
    return masks, boxes, matched


@pytest.mark.parametrize('M', [28, 7])
def test_mask_targets_bit_equal_the_twin(M):
    masks, boxes, matched = mask_case(M)
    grids = [(ref.adaptive_grid(b[1], b[3], M), ref.adaptive_grid(b[0], b[2], M)) for b in boxes]
    assert grids[0][1] == 1 and 1 in grids[1] and 2 in grids[2] and grids[4][0] != grids[4][1] and max(grids[7]) > 4
    want = ref.mask_targets(masks, boxes, matched, M)
    assert want[:8].any() and 0 < want[3].mean() < 1 and not want[9].any()
    R, guard, sentinel = len(boxes), 64, -777.0
    buf = torch.full((R * M * M + 2 * guard,), sentinel, device='cuda')
    m, b, idx = dev(masks), dev(boxes), dev(matched)
    ptrs, dims = dt._mask_tables([m], m.device)
    _lib.check(_lib.lib().cosy_dt_mask_loss(_lib.ptr(ptrs), _lib.ptr(dims), 1, _lib.ptr(b), None, _lib.ptr(idx), None, R, None, 1, M, None, None,
                                            buf.data_ptr() + 4 * guard, None, _lib.stream()))
    got = host(buf)
    assert (got[:guard] == sentinel).all() and (got[-guard:] == sentinel).all()
    inner = got[guard:-guard].reshape(R, M, M)
    assert np.array_equal(inner.view(np.uint32), want.view(np.uint32)), np.abs(inner - want).max()
    assert torch.equal(dt.mask_targets(m, b, idx, M), dev(want))
    # a matched index no mask has: zeros, nothing read
    assert not dt.mask_targets(m, b[:2], dev(np.array([3, -1], np.int32)), M).any()


def test_mask_loss_and_gradient():
    M, C, rows = 28, 3, 6
    masks, boxes, matched = mask_case(M)
    rng = np.random.RandomState(4)
    all_masks = [masks, (rng.uniform(0, 1, (2,) + FRAME) < 0.3).astype(np.uint8)]
    gt = [random_boxes(rng, 3), random_boxes(rng, 2)]
    pos_boxes = np.concatenate([boxes[:rows], boxes[2:2 + rows]])
    pos_matched = np.concatenate([matched[:rows], [0, 1, 0, 1, 0, 1]]).astype(np.int32)
    pos_labels = rng.randint(1, C, 2 * rows).astype(np.int32)
    x = rng.normal(0, 2, (2 * rows, C, M, M)).astype(f32)
    x.reshape(-1)[rng.permutation(x.size)[:x.size // 4]] = np.array([0, 100, -100, 1e4, -1e4], f32)[rng.randint(0, 5, x.size // 4)]
    targets = targets_of(gt, masks=all_masks)
    for counts in ([4, 3], [6, 0], [0, 0]):
        real = np.concatenate([np.arange(rows) < c for c in counts])
        tg = np.concatenate([ref.mask_targets(all_masks[b], pos_boxes[b * rows:(b + 1) * rows], pos_matched[b * rows:(b + 1) * rows], M) for b in range(2)])
        loss64, bound, grad64, n = ref.mask_loss(x, pos_labels, tg, real)
        xx = dev(x).requires_grad_()
        loss = dt.maskrcnn_loss(xx, dev(pos_boxes), dev(pos_labels), dev(pos_matched), targets, dev(np.array(counts, np.int32)))
        (2 * loss).backward()
        g = host(xx.grad).astype(np.float64) / 2
        assert np.isfinite(g).all() and not g[grad64 == 0].any()
        if n == 0:                                                       # no positive: exactly 0, zero gradients
            assert loss.item() == 0.0 and not g.any()
            continue
        share(f'loss_mask counts {counts}', abs(loss.item() - loss64), bound)
        share('grad mask_logits', np.abs(g - grad64), (ref.SIGMOID_GRAD_BOUND + 2 * U) / (n * M * M))
    full = dt.maskrcnn_loss(dev(x), dev(pos_boxes), dev(pos_labels), dev(pos_matched), targets)       # without counts every row is real
    want = ref.mask_loss(x, pos_labels, tg, np.ones(2 * rows, bool))
    share('loss_mask without counts', abs(float(full) - want[0]), want[1])


# ---- RoI training samples and the chain ------------------------------------------------------------------------------------------------
class Heads:
    """tiny heads as torch.nn modules.  The RPN's size deltas are zero, so exp(0) = 1 on both sides and the proposals of the device chain and of
    the twin chain are bit-equal; the box and mask heads run in float64 and round once, so the padded rows and the order of a float32 GEMM's sums
    cannot separate the two sides."""

    def __init__(self, seed=0, C=8, K=3):
        g = torch.Generator().manual_seed(seed)
        self.conv, self.logit, self.delta = torch.nn.Conv2d(C, C, 3, padding=1), torch.nn.Conv2d(C, A, 1), torch.nn.Conv2d(C, 4 * A, 1)
        self.fc, self.cls, self.reg = torch.nn.Linear(C * 49, 16).double(), torch.nn.Linear(16, K).double(), torch.nn.Linear(16, 4 * K).double()
        self.mask = torch.nn.Linear(C, K).double()
        self.modules = (self.conv, self.logit, self.delta, self.fc, self.cls, self.reg, self.mask)
        with torch.no_grad():
            for m in self.modules:
                for p in m.parameters():
                    p.copy_((torch.randn(p.shape, generator=g) * (0.3 if p.dim() > 1 else 0.1)).to(p.dtype))
            self.delta.weight.view(A, 4, C)[:, 2:] = 0
            self.delta.bias.view(A, 4)[:, 2:] = 0
            self.reg.weight *= 0.2
        for m in self.modules:
            m.cuda()
        self.raw = {}

    def parameters(self):
        return [(f'{type(m).__name__}{i}.{n}', p) for i, m in enumerate(self.modules) for n, p in m.named_parameters()]

    def keep(self, name, t):
        if t.requires_grad:
            t.retain_grad()
        self.raw[name] = t
        return t

    def rpn(self, feats):
        hidden = [torch.relu(self.conv(f)) for f in feats]
        return ([self.keep(f'objectness{l}', self.logit(h)) for l, h in enumerate(hidden)],
                [self.keep(f'deltas{l}', self.delta(h)) for l, h in enumerate(hidden)])

    def box(self, roi):
        h = torch.relu(self.fc(roi.flatten(1).double()))
        return self.keep('class_logits', self.cls(h).float()), self.keep('box_regression', self.reg(h).float())

    def mask_head(self, roi):                                            # a 1 x 1 "convolution" as a linear over the channels, in float64
        return self.keep('mask_logits', self.mask(roi.double().permute(0, 2, 3, 1)).permute(0, 3, 1, 2).float().contiguous())

    def numpy(self):
        def rpn(feats):
            with torch.no_grad():
                o, d = self.rpn([dev(f) for f in feats])
            return [host(t) for t in o], [host(t) for t in d]

        def box(roi):
            with torch.no_grad():
                c, r = self.box(dev(roi))
            return host(c), host(r)

        def mask(roi):
            with torch.no_grad():
                return host(self.mask_head(dev(roi)))
        return rpn, box, mask


def chain_case():
    rng = np.random.RandomState(21)
    feats = [rng.normal(0, 1, (2, 8, H, W)).astype(f32) for H, W in GRID]
    gt = [np.array([[8, 0, 40, 32], [20, 10, 50, 36], [0, 0, 20, 18]], f32), np.array([[2, 3, 30, 30], [25, 5, 50, 35]], f32)]
    labels = [[1, 2, 1], [2, 1]]
    masks = [(rng.uniform(0, 1, (len(g), 40, 56)) < 0.5).astype(np.uint8) for g in gt]
    keys = dict(rpn=rng.randint(0, 2 ** 31 - 1, (2, N_ANCHORS)).astype(np.int32), roi=rng.randint(0, 2 ** 31 - 1, (2, 20 + 3)).astype(np.int32))
    return feats, gt, labels, masks, keys


CHAIN_RPN = dict(pre_nms_top_n=64, post_nms_top_n=20)


def test_roi_training_samples_equal_the_twin():
    rng = np.random.RandomState(9)
    _, gt, labels, _, _ = chain_case()
    rows, counts = 40, [40, 17]
    props = np.stack([random_boxes(rng, rows, low=6), random_boxes(rng, rows, low=6)])
    props[0, :8] = gt[0][[0, 1, 2, 0, 1, 2, 0, 1]] + rng.uniform(-1.5, 1.5, (8, 4)).astype(f32)      # proposals close to ground truths
    props[1, 17:] = 0
    for bs, frac in ((512, 0.25), (8, 0.25)):
        keys = rng.randint(0, 2 ** 31 - 1, (2, rows + 3)).astype(np.int32)
        got = dt.roi_training_samples(dev(props.reshape(-1, 4)), dev(np.array(counts, np.int32)), targets_of(gt, labels), keys=dev(keys),
                                      batch_size_per_image=bs, positive_fraction=frac)
        got = {k: host(v) for k, v in got.items()}
        n_pos_max = int(bs * frac)
        for b in range(2):
            want = ref.roi_samples(props[b, :counts[b]], gt[b], labels[b], keys[b], rows, 3, bs, frac)
            n, k = len(want['idx']), len(want['pos_idx'])
            assert (got['counts'][b], got['pos_counts'][b]) == (n, k) and k >= 2 and (want['labels'] == 0).any()
            rows_b = slice(b * bs, b * bs + n)
            assert np.array_equal(got['boxes'][rows_b], want['boxes']) and np.array_equal(got['labels'][rows_b], want['labels'])
            assert np.array_equal(got['matched_idxs'][rows_b], want['matched'])
            with np.errstate(all='ignore'):
                share(f'regression targets image {b}', np.abs(got['regression_targets'][rows_b] - want['targets64']), want['target_bounds'])
            pad = slice(b * bs + n, (b + 1) * bs)
            assert not got['boxes'][pad].any() and (got['labels'][pad] == -1).all() and not got['regression_targets'][pad].any()
            pos_b = slice(b * n_pos_max, b * n_pos_max + k)
            assert np.array_equal(got['pos_boxes'][pos_b], want['pos_boxes']) and np.array_equal(got['pos_labels'][pos_b], want['pos_labels'])
            assert np.array_equal(got['pos_matched_idxs'][pos_b], want['pos_matched'])
            assert (got['pos_labels'][b * n_pos_max + k:(b + 1) * n_pos_max] == -1).all()


def test_detector_losses_equal_the_twin_chain():
    feats, gt, labels, masks, keys = chain_case()
    heads = Heads()
    targets_np = [dict(boxes=g, labels=l, masks=m) for g, l, m in zip(gt, labels, masks)]
    want = ref.chain(feats, heads.numpy(), targets_np, NETS, PAD, SIZES, RATIOS, keys, 2, CHAIN_RPN)
    assert want['pos_real'].sum() >= 4 and (want['labels'] == 0).sum() >= 4 and want['rpn']['n_sampled'] > 20
    heads.raw.clear()
    losses = dt.detector_losses([dev(f) for f in feats], heads.rpn, heads.box, heads.mask_head, targets_of(gt, labels, masks), NETS, PAD, n_roi_levels=2,
                                keys={k: dev(v) for k, v in keys.items()}, sizes=SIZES, aspect_ratios=RATIOS, **CHAIN_RPN)
    assert tuple(losses) == dt.LOSS_KEYS
    for name in dt.LOSS_KEYS:
        share(name, abs(losses[name].item() - want['losses'][name]), want['bounds'][name])
    total = sum(ref.WEIGHTS[k] * losses[k] for k in dt.LOSS_KEYS)         # h_maskrcnn's weighted sum
    total.backward()
    raw = {k: host(v.grad).astype(np.float64) for k, v in heads.raw.items()}
    n_s, frc = want['rpn']['n_sampled'], want['frc']
    for l in range(len(GRID)):
        share(f'chain grad objectness {l}', np.abs(raw[f'objectness{l}'] - want['rpn']['grad_objectness'][l]), (ref.SIGMOID_GRAD_BOUND + 2 * U) / n_s)
        share(f'chain grad deltas {l}', np.abs(raw[f'deltas{l}'] - want['rpn']['grad_deltas'][l]), 3 * U / n_s)
    share('chain grad class_logits', np.abs(raw['class_logits'] - frc['grad_logits']), frc['grad_logits_bound'] + 0 * frc['grad_logits'])
    # the targets of the chain are the float32 encode's: a target within its bound moves a smooth-L1 derivative (slope <= 1) by at most that much
    box_bound = np.full(frc['grad_box'].shape, frc['grad_box_bound'])
    for r in np.flatnonzero(want['labels'] > 0):
        box_bound[r, 4 * want['labels'][r]:4 * want['labels'][r] + 4] += want['target_bounds'][r] / frc['n']
    share('chain grad box_regression', np.abs(raw['box_regression'] - frc['grad_box']), box_bound)
    n_pos, M = int(want['pos_real'].sum()), raw['mask_logits'].shape[-1]
    share('chain grad mask_logits', np.abs(raw['mask_logits'] - want['grad_mask']), (ref.SIGMOID_GRAD_BOUND + 2 * U) / (n_pos * M * M))
    for name, p in heads.parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.any()), name


# ---- the C entry points' refusals ------------------------------------------------------------------------------------------------------
def refusals(name, fn, good, bads):
    """every violation is refused with -1 before any launch; the valid call returns 0"""
    call = lambda **kw: fn(*[kw.get(k, v) for k, v in good.items()])
    assert call() == 0, _lib.lib().cosy_last_error()
    wrong = [(bad, rc) for bad in bads for rc in [call(**bad)] if rc != -1 or not set(bad) <= set(good)]
    torch.cuda.synchronize()
    print(f'{name}: {len(bads)} violations, not refused with -1: {wrong} (bound: none)')
    assert not wrong


def cuda(shape, dtype=torch.float32):
    return torch.zeros(shape if isinstance(shape, tuple) else (shape,), dtype=dtype, device='cuda')


def levels(obj=None, dl=None, **change):
    grid = dt.AnchorGrid(GRID, PAD, SIZES, RATIOS)
    lv = grid.levels(obj, dl)
    for field, (l, v) in change.items():
        getattr(lv, field)[l] = v
    return lv


def test_c_abi_refusals():
    lib, ptr, i32 = _lib.lib(), _lib.ptr, torch.int32
    B, N, bs, npos = 2, N_ANCHORS, 8, 4
    gt, off, gl = cuda((5, 4)), dev(np.array([0, 3, 5], np.int32)), cuda(5, i32) + 1
    gt[:, 2:] = 10
    matched, iou, labels, best = cuda((B, N), i32), cuda((B, N)), cuda((B, N), i32), cuda(5, i32)
    keep = [levels(), levels(H=(1, 0)), levels(W=(2, -3)), levels(H=(0, 1 << 20))]
    by = ctypes.byref
    level_bads = [dict(lv=None), dict(L=0), dict(L=9), dict(A=0), dict(A=17), dict(lv=by(keep[1])), dict(lv=by(keep[2])), dict(lv=by(keep[3]))]
    batch_bads = [dict(B=0), dict(B=2048)]
    good = dict(lv=by(keep[0]), L=3, A=A, cand=None, cc=None, N=N, B=B, gt=ptr(gt), off=ptr(off), gl=None, G_max=3, G_total=5, high=0.7, low=0.3, lq=1,
                best=ptr(best), matched=ptr(matched), iou=ptr(iou), labels=ptr(labels), s=None)
    cand, cc = cuda((B, N, 4)), cuda(B, i32) + 5
    refusals('cosy_dt_match', lib.cosy_dt_match, good, level_bads + batch_bads + [
        dict(N=0), dict(N=N + 1), dict(B=2047, N=1 << 20, cand=ptr(cand)), dict(cc=ptr(cc)), dict(G_max=0), dict(G_max=dt.MAX_GT + 1, G_total=dt.MAX_GT + 1),
        dict(G_total=2), dict(low=0.8), dict(high=float('nan')), dict(gt=None), dict(off=None), dict(matched=None), dict(iou=None), dict(best=None),
        dict(gl=ptr(gl), labels=None)])
    assert lib.cosy_dt_match(None, 0, 0, ptr(cand), ptr(cc), N, B, ptr(gt), ptr(off), ptr(gl), 3, 5, 0.5, 0.5, 0, None, ptr(matched), ptr(iou), ptr(labels),
                             None) == 0                                 # the boxes path needs no levels and no scratch
    keys = cuda((B, N), i32)
    s_idx, s_cnt, p_idx, p_cnt = cuda((B, bs), i32), cuda(B, i32), cuda((B, npos), i32), cuda(B, i32)
    good = dict(labels=ptr(labels), keys=ptr(keys), N=N, B=B, bs=bs, npos=npos, s_idx=ptr(s_idx), s_cnt=ptr(s_cnt), p_idx=ptr(p_idx), p_cnt=ptr(p_cnt), s=None)
    refusals('cosy_dt_sample', lib.cosy_dt_sample, good, batch_bads + [dict(N=0), dict(bs=0), dict(bs=dt.MAX_BATCH + 1), dict(npos=-1), dict(npos=bs + 1)] +
             [{p: None} for p in ('labels', 'keys', 's_idx', 's_cnt', 'p_idx', 'p_cnt')])
    enc = cuda((5, 4))
    good = dict(ref=ptr(gt), boxes=ptr(gt), n=5, wx=1.0, wy=1.0, ww=1.0, wh=1.0, out=ptr(enc), s=None)
    refusals('cosy_dt_encode', lib.cosy_dt_encode, good, [dict(n=-1), dict(n=1 << 29), dict(ref=None), dict(boxes=None), dict(out=None)])
    assert lib.cosy_dt_encode(None, None, 0, 1.0, 1.0, 1.0, 1.0, None, None) == 0
    obj, dl = [cuda((B, A, H, W)) for H, W in GRID], [cuda((B, 4 * A, H, W)) for H, W in GRID]
    g_obj, g_dl = [torch.zeros_like(t) for t in obj], [torch.zeros_like(t) for t in dl]
    full, grads = levels(obj, dl), levels(g_obj, g_dl)
    holes = [levels(obj, dl, objectness=(1, None)), levels(obj, dl, deltas=(2, None)), levels(g_obj, g_dl, objectness=(0, None)), levels(g_obj, g_dl, deltas=(1, None))]
    terms, losses = cuda(2 * B * bs, torch.float64), cuda(2)
    good = dict(lv=by(full), gr=by(grads), L=3, A=A, B=B, bs=bs, s_idx=ptr(s_idx), s_cnt=ptr(s_cnt), matched=ptr(matched), gt=ptr(gt), off=ptr(off),
                terms=ptr(terms), losses=ptr(losses), s=None)
    refusals('cosy_dt_rpn_loss', lib.cosy_dt_rpn_loss, good, level_bads + batch_bads + [dict(bs=0), dict(bs=dt.MAX_BATCH + 1), dict(gr=None),
             dict(lv=by(holes[0])), dict(lv=by(holes[1])), dict(gr=by(holes[2])), dict(gr=by(holes[3]))] +
             [{p: None} for p in ('s_idx', 's_cnt', 'matched', 'gt', 'off', 'terms', 'losses')])
    rows = 6
    props, counts, rc, rcc = cuda((B * rows, 4)), cuda(B, i32) + 4, cuda((B, rows + 3, 4)), cuda(B, i32)
    good = dict(props=ptr(props), counts=ptr(counts), rows=rows, gt=ptr(gt), off=ptr(off), B=B, G_max=3, cand=ptr(rc), cc=ptr(rcc), s=None)
    refusals('cosy_dt_roi_candidates', lib.cosy_dt_roi_candidates, good, batch_bads + [dict(rows=-1), dict(rows=1 << 30), dict(G_max=0), dict(G_max=dt.MAX_GT + 1),
             dict(props=None)] + [{p: None} for p in ('counts', 'gt', 'off', 'cand', 'cc')])
    Nc = rows + 3
    m2, l2 = cuda((B, Nc), i32), cuda((B, Nc), i32)
    outs = dict(boxes=cuda((B * bs, 4)), ol=cuda(B * bs, i32), om=cuda(B * bs, i32), tg=cuda((B * bs, 4)), pb=cuda((B * npos, 4)), pl=cuda(B * npos, i32),
                pm=cuda(B * npos, i32))
    good = dict(cand=ptr(rc), N=Nc, matched=ptr(m2), labels=ptr(l2), s_idx=ptr(s_idx), s_cnt=ptr(s_cnt), p_idx=ptr(p_idx), p_cnt=ptr(p_cnt), gt=ptr(gt),
                off=ptr(off), B=B, bs=bs, npos=npos, wx=10.0, wy=10.0, ww=5.0, wh=5.0, **{k: ptr(v) for k, v in outs.items()}, s=None)
    refusals('cosy_dt_roi_gather', lib.cosy_dt_roi_gather, good, batch_bads + [dict(N=0), dict(bs=0), dict(bs=dt.MAX_BATCH + 1), dict(npos=-1), dict(npos=bs + 1)] +
             [{p: None} for p in ('cand', 'matched', 'labels', 's_idx', 's_cnt', 'p_idx', 'p_cnt', 'gt', 'off', 'boxes', 'ol', 'om', 'tg', 'pb', 'pl', 'pm')])
    R, C = 5, 3
    z, d, lab, t = cuda((R, C)), cuda((R, 4 * C)), cuda(R, i32), cuda((R, 4))
    n_real, terms2, gz, gd = cuda(1, i32), cuda(2 * R, torch.float64), cuda((R, C)), cuda((R, 4 * C))
    good = dict(z=ptr(z), d=ptr(d), lab=ptr(lab), t=ptr(t), R=R, C=C, n_real=ptr(n_real), terms=ptr(terms2), gz=ptr(gz), gd=ptr(gd), losses=ptr(losses), s=None)
    refusals('cosy_dt_fastrcnn_loss', lib.cosy_dt_fastrcnn_loss, good, [dict(R=0), dict(R=1 << 22), dict(C=1), dict(C=dt.MAX_CLASSES + 1)] +
             [{p: None} for p in ('z', 'd', 'lab', 't', 'n_real', 'terms', 'gz', 'gd', 'losses')])
    M, rows = 7, 2
    masks = cuda((3,) + FRAME, torch.uint8)
    mp, md = dt._mask_tables([masks, masks], masks.device)
    x, pb, pl, pm, pc = cuda((B * rows, C, M, M)), cuda((B * rows, 4)), cuda(B * rows, i32) + 1, cuda(B * rows, i32), cuda(B, i32) + 1
    part, gx, tg, loss = cuda(B * rows, torch.float64), cuda((B * rows, C, M, M)), cuda((B * rows, M, M)), cuda(1)
    good = dict(mp=ptr(mp), md=ptr(md), B=B, pb=ptr(pb), pl=ptr(pl), pm=ptr(pm), pc=ptr(pc), rows=rows, x=ptr(x), C=C, M=M, part=ptr(part), gx=ptr(gx), tg=ptr(tg),
                loss=ptr(loss), s=None)
    refusals('cosy_dt_mask_loss', lib.cosy_dt_mask_loss, good, batch_bads + [dict(rows=0), dict(M=0), dict(M=dt.MAX_MASK_SIDE + 1), dict(C=0),
             dict(C=dt.MAX_CLASSES + 1), dict(B=2047, rows=1 << 10, C=64, M=128), dict(mp=None), dict(md=None), dict(pb=None), dict(pm=None), dict(x=None, tg=None),
             dict(pl=None), dict(part=None), dict(gx=None), dict(loss=None)])
