"""The detector's proposal side on the GPU (csrc/kernels_detpre.hip behind cosypose_amd/detector_rpn.py) against the CPU twin
tests/detpre_ref.py, which test_detector_rpn_host.py holds against hand-derived vectors.

Selected anchors, kept (image, candidate index) lists and levels are compared for EQUALITY.  Proposal boxes: within 4 float32 ulps of the
larger coordinate of the box along the axis, section 21's bound (the same rounded operations on both sides, which differ in their exp only).
RoIAlign: BIT-equal to the float32 twin (the same correctly rounded operations in the same order, contraction off), and against the float64
evaluation within the bound derived at test_msroi_align_equals_the_twin."""
import ctypes

import numpy as np
import pytest
import torch

import detpost_ref as post
import detpre_ref as ref
from cosypose_amd import detections_from_features, multiscale_roi_align, rpn_proposals
from cosypose_amd import _lib, detector, detector_rpn
from cosypose_amd.io_formats import make_detections

pytestmark = pytest.mark.gpu
f32 = np.float32

GRID, A = [(5, 7), (3, 4), (1, 2)], 3                               # 105 + 36 + 6 anchors per image
SIZES = ((32,), (64,), (128,))
PAD, NETS, FRAME = (40, 56), [(37, 53), (40, 50)], (24, 40)         # strides 8, 8 / 13.33, 14 / 40, 28: one of them no integer
VALUES = ((np.arange(9) - 4.5) * 0.5).astype(f32)                   # 9 distinct logits, -2.25 .. 1.75: five negative, four positive


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def post_ulps(got, want):
    """|got - want| in float32 ulps of the larger coordinate of the box along the axis (section 21's measure)"""
    got, want = np.asarray(got, f32).reshape(-1, 2, 2), np.asarray(want, f32).reshape(-1, 2, 2)
    mag = np.abs(want).max(1, keepdims=True)
    return np.abs(got.astype(np.float64) - want) / np.spacing(np.maximum(mag, f32(1e-30)))


def grid_case(seed, B=2, grid=GRID, spread=0.5):
    """logits from VALUES (ties everywhere), random deltas; one NaN logit (image 0, level 0) and one NaN delta (last image, level 1)"""
    rng = np.random.RandomState(seed)
    obj = [VALUES[rng.randint(0, 9, (B, A, H, W))] for H, W in grid]
    dl = [(rng.uniform(-1, 1, (B, 4 * A, H, W)) * spread).astype(f32) for H, W in grid]
    obj[0][0, 1, 2, 3] = np.nan
    if len(grid) > 1:
        dl[1][B - 1, 4 * 2 + 1, 1, 2] = np.nan
    return obj, dl


# ---- select --------------------------------------------------------------------------------------------------------------------------
def kernel_order(logits, chosen):
    """the order cosy_rpn_select writes the twin's choice in: strictly above the k-th value by ascending index, then the ties at it"""
    if len(chosen) == 0:
        return []
    kth = logits[chosen[-1]]
    return sorted(int(i) for i in chosen if logits[i] > kth) + sorted(int(i) for i in chosen if logits[i] == kth)


@pytest.mark.parametrize('pre', [1, 4, 64, 1000])                   # below, at (level 2 has 6 anchors, level 1 36) and above a level's count
def test_select_equals_the_twin(pre):
    obj, dl = grid_case(3)
    sel, cnt = detector_rpn.rpn_select([dev(o) for o in obj], [dev(d) for d in dl], pre)
    sel, cnt = sel.cpu().numpy(), cnt.cpu().numpy()
    tied = 0
    for b in range(2):
        want = ref.select(obj, dl, b, pre)
        for l, w in enumerate(want):
            logits = ref.flatten_level(obj[l][b], dl[l][b])[0]
            n = A * GRID[l][0] * GRID[l][1]
            absent = int(np.isnan(logits).sum()) + int(b == 1 and l == 1)
            assert len(w) == min(pre, n - absent) == cnt[b, l]
            assert sel[b, l, :cnt[b, l]].tolist() == kernel_order(logits, w)
            assert (sel[b, l, cnt[b, l]:] == -1).all()                          # nothing written past the count
            got_sorted = sorted(sel[b, l, :cnt[b, l]].tolist(), key=lambda i: (-float(logits[i]), i))
            assert got_sorted == w.tolist()                                     # the twin's order: descending logit, lower index first
            rest = np.setdiff1d(np.arange(n), w)
            tied += int(len(w) > 0 and (logits[rest] == logits[w[-1]]).any())
    assert tied > 0 or pre == 1000                                             # the k-th value is tied with something left out


def test_select_walks_many_chunks_on_keys_that_differ_in_the_low_byte():
    H, W = 100, 234                                                 # 70 200 anchors: 69 chunks of 1024
    rng = np.random.RandomState(5)
    bits = (0xbf800000 + rng.randint(0, 256, (2, A, H, W))).astype(np.uint32)          # -1 - j 2^-23: the first three histogram passes see one bin
    bits[1] = (0x3f800000 + rng.randint(0, 256, (A, H, W))).astype(np.uint32)
    obj = [bits.view(f32)]
    dl = [np.zeros((2, 4 * A, H, W), f32)]
    dl[0][0, 5, 50, 17] = np.nan
    obj[0][1, 2, 99, 233] = np.nan
    sel, cnt = detector_rpn.rpn_select([dev(obj[0])], [dev(dl[0])], 1000)
    sel, cnt = sel.cpu().numpy(), cnt.cpu().numpy()
    for b in range(2):
        w = ref.select(obj, dl, b, 1000)[0]
        logits = ref.flatten_level(obj[0][b], dl[0][b])[0]
        assert cnt[b, 0] == 1000 == len(w)
        assert sel[b, 0].tolist() == kernel_order(logits, w)
        assert (logits == logits[w[-1]]).sum() > (logits[w] == logits[w[-1]]).sum() > 0      # ties at the k-th place, some left out


# ---- proposals -----------------------------------------------------------------------------------------------------------------------
def set_anchor(obj, dl, b, l, y, x, a, logit, deltas):
    obj[l][b, a, y, x] = logit
    dl[l][b, 4 * a:4 * a + 4, y, x] = deltas


def proposal_case():
    """grid_case plus planted anchors with dw = dh = 0 (exp(0) = 1 on both sides: integer boxes) and the highest logits of image 0:
      level 0, a = 1 (32 x 32), cells (0,2), (0,3): boxes [0,0,32,20] and [0,0,32,14] after the clip: IoU 14/20 = fl(0.7), NOT > 0.7: both kept;
      level 1, a = 1 (64 x 64), cell (0,0): [0,0,32,20] again: IoU 1 with the first, another level: kept by the shift;
      level 0, cell (0,0): x2 = 1049 2^-20 (the smallest side the arithmetic can produce that is >= fl32(1e-3): kept) and, in cell (1,0),
      1048 2^-20 (the largest below: dropped).  A side of exactly fl32(1e-3) cannot be produced: with dw = 0 a coordinate next to 16 is a
      multiple of 2^-20, and with any other dw it depends on the last bits of exp."""
    obj, dl = grid_case(11)
    set_anchor(obj, dl, 0, 0, 0, 2, 1, 9.0, [0, 4 / 32, 0, 0])
    set_anchor(obj, dl, 0, 0, 0, 3, 1, 8.5, [-8 / 32, -2 / 32, 0, 0])
    set_anchor(obj, dl, 0, 1, 0, 0, 1, 8.0, [0, -12 / 64, 0, 0])
    set_anchor(obj, dl, 0, 0, 0, 0, 1, 7.5, [(-16 + 1049 * 2.0 ** -20) / 32, 0, 0, 0])
    set_anchor(obj, dl, 0, 0, 1, 0, 1, 7.0, [(-16 + 1048 * 2.0 ** -20) / 32, 0, 0, 0])
    return obj, dl


def check_proposals(obj, dl, nets, got, want, post_n):
    props, counts, scores, levels, src = (t.cpu().numpy() for t in got)
    assert counts.dtype == np.int32 and props.shape == (len(nets) * post_n, 4)
    worst = 0.0
    for b, w in enumerate(want):
        n = int(counts[b])
        rows = slice(b * post_n, b * post_n + n)
        assert n == len(w['src']) and src[rows].tolist() == w['src'].tolist()                  # kept (image, candidate index) lists
        assert levels[rows].tolist() == w['levels'].tolist() and np.array_equal(scores[rows], w['scores'])
        if n:
            worst = max(worst, float(post_ulps(props[rows], w['boxes']).max()))
        pad = slice(b * post_n + n, (b + 1) * post_n)
        assert not props[pad].any() and not scores[pad].any() and (src[pad] == -1).all() and (levels[pad] == -1).all()
    print(f'post_nms_top_n={post_n}: kept {counts.tolist()}, box error {worst:.3g} ulps (bound 4)')
    assert worst <= 4


@pytest.mark.parametrize('post_n', [1, 3, 1000])
def test_proposals_equal_the_twin(post_n):
    obj, dl = proposal_case()
    want = ref.proposals(obj, dl, NETS, PAD, SIZES, pre_nms_top_n=64, post_nms_top_n=post_n)
    args = ([dev(o) for o in obj], [dev(d) for d in dl], NETS, PAD, SIZES)
    got = rpn_proposals(*args, pre_nms_top_n=64, post_nms_top_n=post_n, return_source=True)
    check_proposals(obj, dl, NETS, got, want, post_n)
    if post_n == 1000:
        w0 = want[0]
        first = [3 * (0 * 7 + 2) + 1, 3 * (0 * 7 + 3) + 1, 105 + 1, 3 * 0 + 1, 3 * 7 + 1]     # candidate indices of the planted anchors
        assert w0['src'][:4].tolist() == first[:4] and first[4] not in w0['src'] and first[4] not in w0['candidates']
        assert w0['boxes'][0].tolist() == [0, 0, 32, 20] and w0['boxes'][1].tolist() == [0, 0, 32, 14] and w0['boxes'][2].tolist() == [0, 0, 32, 20]
        assert float(post.iou(post.f32(w0['boxes'][0]), post.f32(w0['boxes'][1]))) == f32(0.7)
        assert w0['boxes'][3][2] == f32(1049 * 2.0 ** -20) >= f32(1e-3) > f32(1048 * 2.0 ** -20)
        for b, (net_h, net_w) in enumerate(NETS):                               # a box clipped at each side of its OWN image
            bx = want[b]['boxes']
            assert (bx[:, 0] == 0).any() and (bx[:, 1] == 0).any() and (bx[:, 2] == net_w).any() and (bx[:, 3] == net_h).any()
            assert len(want[b]['src']) < len(want[b]['candidates'])            # NMS suppressed something
        # the batch's result for each image is bit-equal to that image run alone
        for b in range(2):
            alone = rpn_proposals([dev(o[b:b + 1]) for o in obj], [dev(d[b:b + 1]) for d in dl], NETS[b:b + 1], PAD, SIZES, pre_nms_top_n=64,
                                  post_nms_top_n=post_n, return_source=True)
            for t_all, t_one in zip(got, alone):
                part = t_all[b:b + 1] if t_all.shape[0] == 2 else t_all[b * post_n:(b + 1) * post_n]
                assert torch.equal(part.view(torch.int32) if part.dtype == torch.float32 else part,
                                   t_one.view(torch.int32) if t_one.dtype == torch.float32 else t_one)
        as_list = rpn_proposals(*args, pre_nms_top_n=64, post_nms_top_n=post_n, as_list=True)
        assert [tuple(p.shape) for p in as_list] == [(len(w['src']), 4) for w in want]
        assert torch.equal(as_list[1], got[0][post_n:post_n + len(want[1]['src'])])
        # min_size at exactly the planted side: >= keeps it
        edge = ref.proposals(obj, dl, NETS, PAD, SIZES, pre_nms_top_n=64, post_nms_top_n=post_n, min_size=1049 * 2.0 ** -20)
        assert first[3] in edge[0]['src']
        check_proposals(obj, dl, NETS, rpn_proposals(*args, pre_nms_top_n=64, post_nms_top_n=post_n, min_size=1049 * 2.0 ** -20, return_source=True),
                        edge, post_n)


def test_proposals_of_an_image_whose_every_anchor_is_nan():
    obj, dl = grid_case(13)
    for o in obj:
        o[1] = np.nan
    want = ref.proposals(obj, dl, NETS, PAD, SIZES, pre_nms_top_n=1000, post_nms_top_n=5)
    assert len(want[1]['src']) == 0 and len(want[0]['src']) == 5
    got = rpn_proposals([dev(o) for o in obj], [dev(d) for d in dl], NETS, PAD, SIZES, pre_nms_top_n=1000, post_nms_top_n=5, return_source=True)
    check_proposals(obj, dl, NETS, got, want, 5)
    assert got[1].cpu().tolist() == [5, 0]
    empty = rpn_proposals([dev(o[:0]) for o in obj], [dev(d[:0]) for d in dl], [], PAD, SIZES)
    assert tuple(empty[0].shape) == (0, 4) and tuple(empty[1].shape) == (0,) and empty[0].is_cuda


def test_the_rpn_decoder_and_the_box_head_decoder_agree_to_the_byte():
    """rpn_decode_kernel (weights 1) and det_decode_kernel (weights 10, 10, 5, 5) decode and clip through one box_decode (csrc/det_device.h).
    The same anchors with the same deltas, handed to the box head's side multiplied by its weights, must give the same bytes: the deltas are
    multiples of 1/8 in [-1, 1] (dx, dy in {-1/8, 0, 1/8}, so that no box leaves its image), for which d 10 and d 5 are exact in float32 and
    so is the division back.  One level of 3 x 4 cells with strides 40/3 and 12.5; the second image is smaller, so more of its boxes clip.
    With seed 0 every decoded box keeps sides of at least 1.7 (both CPU twins, which also agree with each other): nothing is dropped by the
    small-box test on either side, and all 2 x 36 anchors must come back from both."""
    H, W, pad, nets, sizes, n = 3, 4, (40, 50), [(40, 50), (38, 47)], ((16,),), 36
    rng = np.random.RandomState(0)
    dl = (rng.randint(-8, 9, (2, 4 * A, H, W)) / 8).astype(f32)
    dl.reshape(2, A, 4, H, W)[:, :, :2] = (rng.randint(-1, 2, (2, A, 2, H, W)) / 8).astype(f32)
    obj = rng.permutation(2 * n).astype(f32).reshape(2, A, H, W)
    anchors = detector_rpn.rpn_anchors([(H, W)], pad, sizes)
    rows = [ref.flatten_level(obj[b], dl[b])[1] for b in range(2)]                             # (36,4) per image, row = anchor index
    for b in range(2):                                                                         # the precondition, on the CPU twins alone
        boxes = post.clip(torch.as_tensor(ref.decode(rows[b], anchors.numpy())), nets[b]).numpy()
        assert min((boxes[:, 2] - boxes[:, 0]).min(), (boxes[:, 3] - boxes[:, 1]).min()) >= 1e-2
        assert 0 < ((boxes[:, :2] == 0).any(1) | (boxes[:, 2] == nets[b][1]) | (boxes[:, 3] == nets[b][0])).sum() < n   # some clip, some do not
    props, counts, _, _, src = rpn_proposals([dev(obj)], [dev(dl)], nets, pad, sizes, pre_nms_top_n=n, post_nms_top_n=n, nms_thresh=1.0,
                                             min_size=1e-2, return_source=True)
    reg = np.concatenate([np.concatenate([np.zeros((n, 4), f32), r * np.array([10, 10, 5, 5], f32)], 1) for r in rows])
    assert (reg[:, 4:] / np.array([10, 10, 5, 5], f32) == np.concatenate(rows)).all()
    logits = np.tile(np.array([0, 20], f32), (2 * n, 1))
    boxes, _, labels, im_ids, cand = detector.postprocess_detections(dev(logits), dev(reg), [anchors.cuda()] * 2, nets, None, nms_thresh=1.0,
                                                                     detections_per_img=64, return_source=True)
    assert counts.cpu().tolist() == [n, n] and tuple(boxes.shape) == (2 * n, 4) and (labels == 1).all()
    props, src, boxes, im_ids, cand = (t.cpu().numpy() for t in (props, src, boxes, im_ids, cand))
    for b in range(2):
        from_rpn, from_head = props[b * n:(b + 1) * n], boxes[im_ids == b]
        by_rpn, by_head = np.argsort(src[b * n:(b + 1) * n]), np.argsort(cand[im_ids == b])
        assert sorted(src[b * n:(b + 1) * n].tolist()) == sorted(cand[im_ids == b].tolist()) == list(range(n))   # every anchor, on both sides
        assert from_rpn[by_rpn].tobytes() == from_head[by_head].tobytes()


# ---- RoIAlign ------------------------------------------------------------------------------------------------------------------------
MS_GRID = [(16, 20), (8, 10), (4, 5), (2, 3)]
MS_NETS = [(64, 80), (60, 70)]                                      # scales 1/4 .. 1/32 from the larger image, k = 2 .. 5
MS_SCALES = [0.25, 0.125, 0.0625, 0.03125]
MS_FEATS = {}


def ms_features(C):
    if C not in MS_FEATS:
        rng = np.random.RandomState(40 + C)
        MS_FEATS[C] = [rng.uniform(-2, 2, (2, C, H, W)).astype(f32) for H, W in MS_GRID]
    return MS_FEATS[C]


def ms_boxes(R):
    special = np.array([[10.3, 8.2, 40.7, 30.9],                    # inside the map (level 0)
                        [-9.5, 10, 18, 31], [20, -7.2, 45, 17.5], [60, 12, 95.4, 40], [12, 40, 38, 75.3],     # across each border
                        [130, 120, 160, 150], [-70, -60, -30, -25],   # wholly outside: every value 0
                        [33.2, 14.1, 33.9, 14.6],                   # smaller than one feature pixel: the clamp to 1
                        [20, 20, 20, 50], [20, 20, 50, 20], [50, 20, 20, 60], [60, 50, 20, 10],                # zero area; inverted in x; in both
                        [5, 5, 9.5, 9.25],                          # the lower clamp of the level mapper
                        [-900, -800, 1100, 1300],                   # the upper clamp
                        [1, 2, 61, 71], [-20, -30, 200, 170], [-100, -100, 200, 250]], f32)                    # levels 0, 1, 2 unclamped
    rng = np.random.RandomState(R)
    x1, y1 = rng.uniform(-10, 70, 65), rng.uniform(-10, 55, 65)
    rand = np.stack([x1, y1, x1 + rng.uniform(2, 300, 65), y1 + rng.uniform(2, 300, 65)], 1).astype(f32)
    boxes = np.concatenate([special, rand])[:R] if R > 1 else special[:R]
    return boxes, (np.arange(len(boxes)) % 2).astype(np.int64)      # the two images interleaved


def msroi_direct(feats, boxes, im_ids, P, g, guard=64, sentinel=-777.0):
    """the C entry point on a sentinel-filled buffer with guard elements behind it -> out (R,C,P,P), levels, guard untouched"""
    R, C = len(boxes), feats[0].shape[1]
    lv = _lib.MsroiLevels()
    for l, t in enumerate(feats):
        lv.feat[l], lv.H[l], lv.W[l], lv.scale[l] = t.data_ptr(), t.shape[2], t.shape[3], MS_SCALES[l]
    buf = torch.full((R * C * P * P + guard,), sentinel, dtype=torch.float32, device='cuda')
    levels = torch.full((R + guard,), -9, dtype=torch.int32, device='cuda')
    b, i = dev(boxes), dev(im_ids.astype(np.int32))
    rc = _lib.lib().cosy_msroi_align(ctypes.byref(lv), 4, 2, C, _lib.ptr(b), _lib.ptr(i), None, 0, R, P, g, 2, 5, _lib.ptr(buf), _lib.ptr(levels), None)
    assert rc == 0
    torch.cuda.synchronize()
    buf, levels = buf.cpu().numpy(), levels.cpu().numpy()
    assert (buf[R * C * P * P:] == sentinel).all() and (levels[R:] == -9).all()        # no guard element touched
    return buf[:R * C * P * P].reshape(R, C, P, P), levels[:R]


@pytest.mark.parametrize('R', [0, 1, 65])
@pytest.mark.parametrize('g', [1, 2])
@pytest.mark.parametrize('P', [7, 14])
@pytest.mark.parametrize('C', [1, 3, 64, 67])
def test_msroi_align_equals_the_twin(C, P, g, R):
    """Bit-equal to the float32 twin.  Against roi_align64 (weights, products and sums in float64 at the float32 sample positions, which the
    contract fixes: a position is discontinuous at -1 and at `size`, so it is an input of the bilinear sum, not part of its rounding error)
    the bound per value is  u (g^2 + 8) sum |w p| / g^2,  u = 2^-24, first order, times 1 + 2^-10 for the rest.  Count per tap term w p of one
    sample: the low weight h = fl(1 - l) (l = y - floor(y) is exact) 1 rounding, so a weight product fl(hy hx) carries at most 3 (two
    factors, the product), the product with p 1 more: 4; the three additions of a sample's four terms at most 3 more on a term; the
    accumulation over the g^2 samples at most g^2 - 1 additions; the division 1: 4 + 3 + (g^2 - 1) + 1 < g^2 + 8.  The issue allows
    u (7 g^2 + 2) sum |w p| / g^2: 9 u for g = 1 (the same) and 30 u for g = 2, where this derivation gives 12 u; the tighter one is asserted."""
    feats = ms_features(C)
    boxes, im_ids = ms_boxes(R)
    value = ref.level_value64(boxes)
    assert (np.abs(value - np.round(value))[~np.isnan(value)] >= 1e-4).all()   # no box next to a level boundary (NaN: a negative area, level 0)
    want, want_levels = ref.multiscale_roi_align(feats, boxes, im_ids, MS_SCALES, P, g)
    got, levels = msroi_direct([dev(t) for t in feats], boxes, im_ids, P, g)
    assert levels.tolist() == want_levels.tolist()
    assert (got != -777.0).all()                                                # every element written
    assert np.array_equal(got.view(np.int32), want.view(np.int32))             # bit for bit
    if R == 0:
        assert tuple(multiscale_roi_align([dev(t) for t in feats], dev(boxes), MS_NETS, P, g, batch_im_id=dev(im_ids)).shape) == (0, C, P, P)
        return
    v64, _, mag = ref.multiscale_roi_align(feats, boxes, im_ids, MS_SCALES, P, g, np.float64)
    bound = 2.0 ** -24 * (g * g + 8) * (1 + 2.0 ** -10) * mag
    err = np.abs(got.astype(np.float64) - v64)
    print(f'C={C} P={P} g={g} R={R}: max error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3g} (must be <= 1), levels {np.bincount(want_levels, minlength=4).tolist()}')
    assert (err <= bound).all()
    if R == 65:
        assert set(want_levels.tolist()) == {0, 1, 2, 3} and want_levels[12] == 0 and want_levels[13] == 3
        assert not want[5].any() and not want[6].any() and want[0].any() and want[7].any() and want[8].any()
        wrapped, wl = multiscale_roi_align([dev(t) for t in feats], dev(boxes), MS_NETS, P, g, batch_im_id=dev(im_ids), return_levels=True)
        assert np.array_equal(wrapped.cpu().numpy().view(np.int32), got.view(np.int32)) and wl.cpu().tolist() == levels.tolist()
        by_image = [dev(boxes[im_ids == b]) for b in range(2)]                  # the list form and host counts: image by image
        listed = multiscale_roi_align([dev(t) for t in feats], by_image, MS_NETS, P, g).cpu().numpy()
        assert np.array_equal(listed.view(np.int32), np.concatenate([got[im_ids == b] for b in range(2)]).view(np.int32))


def test_msroi_align_padded_rows_and_bad_image_ids():
    feats, (boxes, _) = ms_features(3), ms_boxes(65)
    t = [dev(x) for x in feats]
    rows = 8                                                        # image b owns rows [8 b, 8 b + 8), counts 5 and 0
    counts = dev(np.array([5, 0], np.int32))
    got, levels = multiscale_roi_align(t, dev(boxes[:16]), MS_NETS, 7, 2, counts=counts, return_levels=True)
    want, wl = ref.multiscale_roi_align(feats, boxes[:5], np.zeros(5, np.int64), MS_SCALES, 7, 2)
    assert np.array_equal(got[:5].cpu().numpy().view(np.int32), want.view(np.int32)) and levels[:5].cpu().tolist() == wl.tolist()
    assert not got[5:].any() and (levels[5:] == -1).all()
    ids = np.array([0, 1, 2, -1, 1], np.int64)                      # an image id outside [0, B): zeros, level -1, nothing read
    got, levels = multiscale_roi_align(t, dev(boxes[:5]), MS_NETS, 7, 2, batch_im_id=dev(ids), return_levels=True)
    assert not got[2:4].any() and levels.cpu().tolist()[2:4] == [-1, -1] and got[4].any()


# ---- the chain -------------------------------------------------------------------------------------------------------------------------
class Heads:
    def __init__(self, seed=0, C=8, K=3, background=0.0):
        g = torch.Generator().manual_seed(seed)
        mk = lambda m: m.cuda().eval().requires_grad_(False)
        self.conv, self.logit, self.delta = mk(torch.nn.Conv2d(C, C, 3, padding=1)), mk(torch.nn.Conv2d(C, A, 1)), mk(torch.nn.Conv2d(C, 4 * A, 1))
        self.fc, self.cls, self.reg = (mk(m.double()) for m in (torch.nn.Linear(C * 49, 16), torch.nn.Linear(16, K), torch.nn.Linear(16, 4 * K)))
        self.mask = mk(torch.nn.Conv2d(C, K, 3, padding=1))
        for m in (self.conv, self.logit, self.delta, self.fc, self.cls, self.reg, self.mask):
            for p in m.parameters():
                p.copy_((torch.randn(p.shape, generator=g) * (0.3 if p.dim() > 1 else 0.1)).to(p.dtype))
        # the size deltas of the RPN are zero: exp(0) = 1 on both sides, so the proposals are bit-equal and everything behind them sees the
        # same inputs on both sides -- section 21's tolerances then apply to the chain unchanged
        self.delta.weight.view(A, 4, C)[:, 2:] = 0
        self.delta.bias.view(A, 4)[:, 2:] = 0
        self.cls.weight *= 8
        self.reg.weight *= 0.2
        if background:                                              # the class logits are their biases: background everywhere
            self.cls.weight.zero_()
        self.cls.bias[0] += background

    def rpn(self, feats):
        hidden = [torch.relu(self.conv(f)) for f in feats]
        return [self.logit(h) for h in hidden], [self.delta(h) for h in hidden]

    def box(self, roi):
        # the two linears run in float64 and round once to float32: the device chain hands them the padded rows too, the twin only the real
        # ones, and a float32 GEMM may sum a row in another order for another batch size
        h = torch.relu(self.fc(roi.flatten(1).double()))
        return self.cls(h).float(), self.reg(h).float()

    # the same modules for the twin chain: numpy in, numpy out
    def rpn_np(self, feats):
        o, d = self.rpn([dev(f) for f in feats])
        return [t.cpu().numpy() for t in o], [t.cpu().numpy() for t in d]

    def box_np(self, roi):
        c, r = self.box(dev(roi))
        return c.cpu().numpy(), r.cpu().numpy()

    def mask_np(self, roi):
        return self.mask(dev(roi)).cpu().numpy()


def chain_features(seed=21, C=8):
    rng = np.random.RandomState(seed)
    return [rng.normal(0, 1, (2, C, H, W)).astype(f32) for H, W in GRID]


NAMES = {1: 'obj_000001', 2: 'obj_000002'}
OPTIONS = dict(sizes=SIZES, pre_nms_top_n=64, post_nms_top_n=20, detections_per_img=100)


@pytest.mark.parametrize('output_masks', [False, True])
def test_detections_from_features_equal_the_twin_chain(output_masks):
    with torch.no_grad():
        heads, feats = Heads(), chain_features()
        twin, props, per_image = ref.chain(feats, heads.rpn_np, heads.box_np, heads.mask_np, NETS, PAD, [FRAME] * 2, NAMES, output_masks=output_masks,
                                           rpn_options=dict(sizes=SIZES, pre_nms_top_n=64, post_nms_top_n=20), head_options=dict(detections_per_img=100))
        got = detections_from_features([dev(f) for f in feats], heads.rpn, heads.box, heads.mask, NETS, PAD, [FRAME] * 2, NAMES,
                                       output_masks=output_masks, **OPTIONS)
    assert len(twin['score']) > 3 and len(set(twin['batch_im_id'].tolist())) == 2 and len(set(twin['label'].tolist())) == 2
    s64 = np.concatenate([post.scores64(heads.box_np(ref.multiscale_roi_align(feats, p['boxes'], np.full(len(p['boxes']), b), ref.infer_scales(
        [f.shape[2:] for f in feats], NETS), 7, 2)[0])[0])[:, 1:].numpy().reshape(-1) for b, p in enumerate(props)])
    assert int((np.abs(s64 - 0.05) < 1e-4).sum()) == 0                         # no score too close to the threshold to call
    fed = [dict(boxes=o['boxes'], labels=[NAMES[int(l)] for l in o['labels']], scores=o['scores']) for o in per_image]
    want = make_detections(fed, device='cuda')
    assert got.infos['batch_im_id'].tolist() == want.infos['batch_im_id'].tolist() == twin['batch_im_id'].tolist()
    assert got.infos['label'].tolist() == want.infos['label'].tolist()
    assert np.abs(got.infos['score'].values / want.infos['score'].values - 1).max() <= (3 + 4 + 16) * 2.0 ** -24 * 2
    assert post_ulps(got.bboxes.cpu().numpy(), want.bboxes.cpu().numpy()).max() <= 5           # section 21: 4 of the decode, 1 of the step to the frame
    assert hasattr(got, 'masks') == output_masks
    if output_masks:
        boxes_net = np.array([per_image[b]['boxes_net'][j] for b, j in twin['rows']], f32).reshape(-1, 4)
        labels = np.array([per_image[b]['labels'][j] for b, j in twin['rows']], np.int64)
        roi = ref.multiscale_roi_align(feats, boxes_net, twin['batch_im_id'], ref.infer_scales([f.shape[2:] for f in feats], NETS), 14, 2)[0]
        v64, inside = post.paste_values(heads.mask_np(roi), twin['bboxes'], labels, FRAME, torch.float64)
        close = ((v64 - 0.8).abs() <= 1e-5).numpy() & inside.numpy()
        D = len(labels)
        assert (close.reshape(D, -1).sum(1) <= 1e-3 * inside.numpy().reshape(D, -1).sum(1)).all()      # the exclusion cap, on the twin alone
        masks = got.masks.cpu().numpy()
        assert masks.dtype == bool and masks.shape == (D,) + FRAME and twin['masks'].any()
        assert not ((masks != twin['masks']) & ~close).any()


def test_detections_from_features_with_nothing_found_and_with_no_image():
    with torch.no_grad():
        heads, feats = Heads(background=60.0), chain_features()

        def no_mask(roi):
            raise AssertionError('no detection, no mask head')
        got = detections_from_features([dev(f) for f in feats], heads.rpn, heads.box, no_mask, NETS, PAD, [FRAME] * 2, NAMES, output_masks=True, **OPTIONS)
        want = make_detections([dict(boxes=np.zeros((0, 4), f32), labels=[], scores=np.zeros(0, f32))] * 2, device='cuda', output_masks=True)
        assert len(got.infos) == 0 and list(got.infos.columns) == list(want.infos.columns)
        assert tuple(got.bboxes.shape) == (0, 4) and got.bboxes.is_cuda and not hasattr(got, 'masks')

        def no_head(*a):
            raise AssertionError('no image, no head')
        none = detections_from_features([dev(f[:0]) for f in feats], no_head, no_head, no_head, [], PAD, [], NAMES, **OPTIONS)
        assert len(none.infos) == 0 and list(none.infos.columns) == list(want.infos.columns) and tuple(none.bboxes.shape) == (0, 4)


# ---- the C entry points' refusals ------------------------------------------------------------------------------------------------------
class Call:
    """a C entry point with a valid argument list by name; refused(name=value, ...) replaces some and reports (return code, outputs untouched)"""

    def __init__(self, fn, outputs, **args):
        self.fn, self.outputs, self.args = fn, outputs, args

    def __call__(self, **kw):
        assert set(kw) <= set(self.args), set(kw) - set(self.args)
        return self.fn(*[kw.get(k, v) for k, v in self.args.items()])

    def check(self, name, bads, noops):
        for t in self.outputs:
            t.fill_(7)
        assert self() == 0
        torch.cuda.synchronize()
        assert not all(bool((t == 7).all()) for t in self.outputs)             # the valid call does write
        wrong = []
        for bad in bads:
            for t in self.outputs:
                t.fill_(7)
            rc = self(**bad)
            torch.cuda.synchronize()
            if rc != -1 or not all(bool((t == 7).all()) for t in self.outputs):
                wrong.append((bad, rc))
        print(f'{name}: {len(bads)} violations, not refused with -1 and untouched outputs: {wrong} (bound: none)')
        assert not wrong
        for noop in noops:
            for t in self.outputs:
                t.fill_(7)
            assert self(**noop) == 0, noop
            torch.cuda.synchronize()
            assert all(bool((t == 7).all()) for t in self.outputs), noop


def cuda(shape, dtype=torch.float32):
    return torch.zeros(shape if isinstance(shape, tuple) else (shape,), dtype=dtype, device='cuda')


def rpn_levels(obj, dl, **change):
    """a valid cosy_rpn_levels_t over device tensors; change: field -> (level, value)"""
    lv = _lib.RpnLevels()
    for l, (o, d) in enumerate(zip(obj, dl)):
        lv.objectness[l], lv.deltas[l], lv.H[l], lv.W[l], lv.stride_h[l], lv.stride_w[l] = o.data_ptr(), d.data_ptr(), o.shape[2], o.shape[3], 8.0, 8.0
        for a in range(A):
            for c in range(4):
                lv.base[l][a][c] = (-16.0, -16.0, 16.0, 16.0)[c]
    for field, (l, v) in change.items():
        getattr(lv, field)[l] = v
    return ctypes.byref(lv)


def test_c_abi_rpn_refusals():
    lib, ptr, i32, i64 = _lib.lib(), _lib.ptr, torch.int32, torch.int64
    obj, dl = grid_case(1)
    obj, dl = [dev(np.nan_to_num(o)) for o in obj], [dev(np.nan_to_num(d)) for d in dl]
    B, L, pre, cap, keep = 2, 3, 8, 64, 4
    good = rpn_levels(obj, dl)
    level_bads = [dict(lv=None), dict(L=0), dict(L=9), dict(A=0), dict(A=17), dict(B=-1), dict(B=2048), dict(pre=0), dict(pre=16384 // 3 + 1),
                  dict(lv=rpn_levels(obj, dl, H=(1, 0))), dict(lv=rpn_levels(obj, dl, W=(2, -3))), dict(lv=rpn_levels(obj, dl, H=(0, 1 << 20))),
                  dict(lv=rpn_levels(obj, dl, objectness=(1, None))), dict(lv=rpn_levels(obj, dl, deltas=(2, None)))]
    sel, cnt = cuda((B, L, pre), i32), cuda((B, L), i32)
    call = Call(lib.cosy_rpn_select, [sel, cnt], lv=good, L=L, A=A, B=B, pre=pre, sel=ptr(sel), cnt=ptr(cnt), s=None)
    call.check('cosy_rpn_select', level_bads + [dict(sel=None), dict(cnt=None)], [dict(B=0, sel=None, cnt=None)])
    assert call() == 0
    net = dev(np.array(NETS, f32).reshape(-1))
    outs = [cuda((B * cap, 4)), cuda(B * cap), cuda(B * cap, i32), cuda(B * cap, i32), cuda(B * cap, i64), cuda(B, i32), cuda(B)]
    call = Call(lib.cosy_rpn_decode, outs, lv=good, L=L, A=A, B=B, pre=pre, sel=ptr(sel), cnt=ptr(cnt), net=ptr(net), min_size=1e-3, cap=cap,
                boxes=ptr(outs[0]), scores=ptr(outs[1]), level=ptr(outs[2]), src=ptr(outs[3]), keys=ptr(outs[4]), counts=ptr(outs[5]),
                max_coord=ptr(outs[6]), s=None)
    pointers = ['sel', 'cnt', 'net', 'boxes', 'scores', 'level', 'src', 'keys', 'counts', 'max_coord']
    bads = level_bads + [dict(cap=0), dict(cap=100), dict(cap=16384 + 64), dict(cap=-64), dict(pre=22), dict(min_size=-1.0), dict(min_size=float('nan'))]
    call.check('cosy_rpn_decode', bads + [{p: None} for p in pointers], [dict(B=0, **{p: None for p in pointers})])
    assert call() == 0
    order = torch.sort(outs[4])[1]
    seg = dev(np.arange(B, dtype=np.int32) * cap)
    from cosypose_amd import detector
    kept, n_kept = detector._nms_segments(outs[0], order, outs[2], outs[6], seg, outs[5], B, cap, 0.7, keep)
    gat = [cuda((B * keep, 4)), cuda(B * keep), cuda(B * keep, i32), cuda(B * keep, i32), cuda(B, i32)]
    call = Call(lib.cosy_rpn_gather, gat, kept=ptr(kept), n_kept=ptr(n_kept), boxes=ptr(outs[0]), scores=ptr(outs[1]), level=ptr(outs[2]), src=ptr(outs[3]),
                B=B, cap=cap, keep=keep, props=ptr(gat[0]), pscores=ptr(gat[1]), plevels=ptr(gat[2]), psrc=ptr(gat[3]), counts=ptr(gat[4]), s=None)
    pointers = ['kept', 'n_kept', 'boxes', 'scores', 'level', 'src', 'props', 'pscores', 'plevels', 'psrc', 'counts']
    bads = [dict(B=-1), dict(B=2048), dict(keep=-1), dict(cap=0), dict(cap=16384 + 64), dict(B=2047, keep=1 << 20)] + [{p: None} for p in pointers]
    call.check('cosy_rpn_gather', bads, [dict(B=0, **{p: None for p in pointers})])
    assert call() == 0
    assert gat[4].cpu().tolist() == n_kept.cpu().tolist()


def test_c_abi_msroi_align_refusals():
    lib, ptr, i32 = _lib.lib(), _lib.ptr, torch.int32
    feats = [dev(t) for t in ms_features(3)]
    boxes, im_ids = ms_boxes(65)
    R, C, P = 6, 3, 7
    b, ids, counts = dev(boxes[:R]), dev(im_ids[:R].astype(np.int32)), dev(np.array([3, 2], np.int32))

    def levels(**change):
        lv = _lib.MsroiLevels()
        for l, t in enumerate(feats):
            lv.feat[l], lv.H[l], lv.W[l], lv.scale[l] = t.data_ptr(), t.shape[2], t.shape[3], MS_SCALES[l]
        for field, (l, v) in change.items():
            getattr(lv, field)[l] = v
        return ctypes.byref(lv)
    out, lvl = cuda((R, C, P, P)), cuda(R, i32)
    call = Call(lib.cosy_msroi_align, [out, lvl], lv=levels(), L=4, B=2, C=C, boxes=ptr(b), im_id=ptr(ids), counts=None, rows=0, R=R, P=P, g=2, k_min=2,
                k_max=5, out=ptr(out), levels=ptr(lvl), s=None)
    bads = [dict(lv=None), dict(L=0), dict(L=9), dict(B=-1), dict(R=-1), dict(C=0), dict(g=0), dict(g=-2), dict(P=0), dict(P=65), dict(P=7, g=19),
            dict(k_min=6), dict(k_max=6), dict(im_id=None), dict(rows=3), dict(im_id=None, rows=0, counts=ptr(counts)), dict(counts=ptr(counts)),
            dict(B=0), dict(lv=levels(H=(1, 0))), dict(lv=levels(W=(3, -1))), dict(lv=levels(H=(0, 1 << 15), W=(0, 1 << 15))), dict(lv=levels(scale=(2, 0.0))),
            dict(lv=levels(scale=(0, float('nan')))), dict(lv=levels(feat=(3, None))), dict(boxes=None), dict(out=None), dict(C=1 << 20, P=64, g=1)]
    call.check('cosy_msroi_align', bads, [dict(R=0, boxes=None, im_id=None, rows=1, out=None, levels=None), dict(R=0, B=0, rows=1, im_id=None)])
    assert call(im_id=None, rows=3, counts=ptr(counts)) == 0 and call(levels=None) == 0
