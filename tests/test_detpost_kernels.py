"""The detector's output kernels (csrc/kernels_detpost.hip behind cosypose_amd/detector.py: decode, NMS, gather, mask paste; DESIGN.md
section 21) at the limits their host checks allow and on edge inputs.  tests/test_detector_post.py holds the ordinary middle of the
input space; this file goes where the kernels' loops, bit fields and store paths change.

Yardsticks and bounds, group by group.  Every test prints its measured figure next to its bound before it asserts.

  NMS      The keep set is defined to the bit (box_iou of csrc/det_device.h, one IEEE rounding per operation), so the yardstick is the
           twin's float32 greedy NMS (detpost_ref.nms_fast, held against the loop of detpost_ref.nms on the CPU) and the bound is
           EQUALITY of the keep lists: 0 differing entries.  What makes an input worth running is asserted on the twin alone (something
           kept, something suppressed, a box suppressed only from two row blocks back, a decision the label shift's rounding changes).
  Decode   ids, labels, image ids, candidate indices: equality with the twin.  Boxes twice: against detpost_ref.decode64 / clip64 (float64)
           within the per-coordinate bound derived in decode64's docstring from the rounding sequence,
           u (|x| + |pcx| + 3 |dx w| + 0.5 |w| + |cx| + (|dw| + 4)/2 pw) (1 + 2^-10), u = 2^-24; and against the float32 twin within the 4 ulps
           of test_detector_post.py.  Frame boxes: bit for bit boxes_net x ratio of THAT image.  Scores: within (C + 4 + 16) 2^-24 relative
           of the float64 softmax.  The inputs keep every float64 score at least 1e-4 away from score_thresh, so the candidate set is
           not a matter of rounding; where scores are meant to be equal they are equal bits on both sides.
  Paste    detpost_ref.paste_value64, a direct per-pixel float64 evaluation of step 8 (F.interpolate cannot state several of these cases):
           equality with value > mask_th on every pixel whose float64 value is farther than 1e-5 from mask_th; at most 0.1 % of a mask's
           in-box pixels may be that close, asserted on the reference alone (also on the CPU, in test_detector_post_host.py).  A pixel
           outside the box holds 0 and is 0 > mask_th like any other (true for a negative mask_th, false for NaN).
  C ABI    every COSY_REQUIRE of the five entry points violated once: return code -1, every output still at its fill value after a
           synchronise; the documented no-op forms return 0."""
import functools
import math

import numpy as np
import pytest
import torch

import detpost_ref as ref
from cosypose_amd import batched_nms, nms, paste_masks, postprocess_detections
from cosypose_amd import detector
from test_detector_post import dev, ulps

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NAN, INF = float('nan'), float('inf')
f32 = np.float32


def boom():
    raise AssertionError('the library was reached by a call that had to be refused before')


def fractional(boxes):
    """non-integer boxes: (all but a stray coordinate in ten thousand) have a fractional part"""
    return bool((boxes != np.round(boxes)).mean() > 0.999)


# ==== NMS ===========================================================================================================================
@functools.lru_cache(maxsize=None)
def case_nms_sizes(N):
    boxes, scores, labels = ref.nms_clustered_case(N)
    assert fractional(boxes)
    want, last = ref.nms_fast(boxes, scores, 0.5, trace=True)
    assert 0 < len(want) < N
    pos = np.arange(N)
    far = int(((last >= 0) & (last // 64 <= pos // 64 - 2)).sum())          # suppressed, and by nothing nearer than two row blocks back
    assert far > 0 or N < 321                                               # (127 .. 129 boxes have too few blocks for it)
    want_b = ref.batched_nms_fast(boxes, scores, labels, 0.5)
    assert len(want) < len(want_b) < N
    return boxes, scores, labels, want, want_b, far


@pytest.mark.parametrize('N', [127, 128, 129, 321, 4097, 16384])
def test_nms_on_float_boxes_equals_the_twin(N):
    boxes, scores, labels, want, want_b, far = case_nms_sizes(N)
    got = nms(dev(boxes), dev(scores), 0.5).cpu().numpy()
    got_b = batched_nms(dev(boxes), dev(scores), dev(labels), 0.5).cpu().numpy()
    wrong = int(len(got) != len(want) or (got != want).sum()) + int(len(got_b) != len(want_b) or (got_b != want_b).sum())
    print(f'N={N}: kept {len(want)} (with labels {len(want_b)}), {far} boxes suppressed only from >= 2 row blocks back; '
          f'keep lists differing from the twin {wrong} (bound 0)')
    assert got.tolist() == want.tolist()
    assert got_b.tolist() == want_b.tolist()


def test_nms_refuses_more_boxes_than_the_cap_before_any_launch(monkeypatch):
    n = detector.MAX_CANDIDATES + 1
    assert n == 16385
    b, s, l = torch.zeros((n, 4), device='cuda'), torch.zeros(n, device='cuda'), torch.zeros(n, dtype=torch.int64, device='cuda')
    monkeypatch.setattr(detector._lib, 'lib', boom)
    with pytest.raises(ValueError, match='16385 boxes exceed the cap of 16384'):
        nms(b, s, 0.5)
    with pytest.raises(ValueError, match='16385 boxes exceed the cap of 16384'):
        batched_nms(b, s, l, 0.5)


@functools.lru_cache(maxsize=None)
def case_nms_labels():
    boxes, scores, labels = ref.nms_label_case()
    assert labels.max() == 4095 and labels.min() == 0 and boxes.max() == f32(999.73) and fractional(boxes)
    want = ref.batched_nms_fast(boxes, scores, labels, 0.5)
    exact = ref.nms64_per_label(boxes, scores, labels, 0.5)
    flipped = len(set(want.tolist()) ^ set(exact))
    assert flipped > 0 and 0 < len(want) < len(boxes)                       # the rounding of the shifted coordinates decides something here
    # ... and so does the rounding of the product label * (max + 1) on its own: a shift contracted into one fused multiply-add keeps another set
    unit = np.float64(boxes.max() + f32(1))
    fused = (boxes.astype(np.float64) + (labels.astype(np.float64) * unit)[:, None]).astype(f32)
    assert ref.nms_fast(fused, scores, 0.5).tolist() != want.tolist()
    neg = (boxes - f32(2000)).astype(f32)
    assert neg.max() < 0
    want_neg = ref.batched_nms_fast(neg, scores, labels % 4, 0.5)
    assert 0 < len(want_neg) < len(boxes)
    return boxes, scores, labels, want, flipped, neg, want_neg


def test_batched_nms_with_labels_up_to_4095_rounds_like_the_twin():
    boxes, scores, labels, want, flipped, neg, want_neg = case_nms_labels()
    got = batched_nms(dev(boxes), dev(scores), dev(labels), 0.5).cpu().numpy()
    got_neg = batched_nms(dev(neg), dev(scores), dev(labels % 4), 0.5).cpu().numpy()
    print(f'labels to 4095: kept {len(want)} of {len(boxes)}, {flipped} decisions differ from an unshifted float64 per-label NMS; all-negative '
          f'coordinates: kept {len(want_neg)}; entries differing from the twin '
          f'{int((got != want).sum()) if len(got) == len(want) else -1} and {int((got_neg != want_neg).sum()) if len(got_neg) == len(want_neg) else -1} (bound 0)')
    assert got.tolist() == want.tolist()
    assert got_neg.tolist() == want_neg.tolist()


#               A                 touches A (intersection 0)   identical to A      disjoint           IoU 1/2 with A
THRESH_BOXES = [[0, 0, 10, 10], [10, 0, 20, 10],              [0, 0, 10, 10],     [50, 50, 60, 60],  [0, 0, 10, 5]]
THRESH_WANT = {0.0: [0, 1, 3],            # 0 > 0 is false: the touching and the disjoint box survive, IoU 1 and 1/2 go
               1.0: [0, 1, 2, 3, 4],      # nothing is > 1: the identical box survives
               -1.0: [0],                 # every IoU here is a number >= 0 > -1
               NAN: [0, 1, 2, 3, 4]}      # nothing is > NaN


@pytest.mark.parametrize('thr', [0.0, 1.0, -1.0, NAN])
def test_nms_thresholds_at_their_ends(thr):
    boxes, scores = np.array(THRESH_BOXES, f32), np.array([.9, .8, .7, .6, .5], f32)
    want = THRESH_WANT[thr]
    assert ref.nms(boxes, scores, thr).tolist() == want and ref.nms_fast(boxes, scores, thr).tolist() == want
    got = nms(dev(boxes), dev(scores), thr).cpu().tolist()
    got_b = batched_nms(dev(boxes), dev(scores), dev(np.zeros(5, np.int64)), thr).cpu().tolist()
    print(f'iou_threshold={thr}: kept {got}, by hand {want} (bound: equal)')
    assert got == want and got_b == want


@functools.lru_cache(maxsize=None)
def case_nms_degenerate():
    boxes, scores, _ = ref.nms_clustered_case(130)
    odd = {0: [5, 5, 5, 9], 20: [100, 100, 100, 100], 21: [100, 100, 100, 100],          # zero area; twice the same point: IoU 0/0
           63: [30, 0, 10, 10], 70: [10, 30, 30, 5], 71: [30, 30, 10, 5],              # inverted in x, in y, in both
           65: [NAN, 0, 10, 10], 100: [0, 0, INF, INF], 129: [-INF, -INF, INF, INF]}
    for i, b in odd.items():
        boxes[i] = b
    boxes[64] = [10, 0, 30, 10]                                                        # an ordinary box right on the inverted one
    want = ref.nms_fast(boxes, scores, 0.5)
    assert want.tolist() == ref.nms(boxes, scores, 0.5).tolist()
    assert set(odd) <= set(want.tolist())                                              # never suppressed
    rest = np.array([i for i in range(130) if i not in odd])
    alone = rest[ref.nms_fast(boxes[rest], scores[rest], 0.5)]
    assert [i for i in want.tolist() if i not in odd] == alone.tolist() and len(alone) < len(rest)      # never suppress
    return boxes, scores, want, sorted(odd)


def test_nms_degenerate_boxes_neither_suppress_nor_are_suppressed():
    boxes, scores, want, odd = case_nms_degenerate()
    got = nms(dev(boxes), dev(scores), 0.5).cpu().tolist()
    print(f'degenerate boxes {odd}: all kept {set(odd) <= set(got)}; entries differing from the twin '
          f'{sum(a != b for a, b in zip(got, want.tolist())) + abs(len(got) - len(want))} (bound 0)')
    assert got == want.tolist()
    # one NaN coordinate anywhere: boxes.max() is NaN, every shift is NaN, every IoU is NaN, everything is kept
    clean, cs, labels = ref.nms_clustered_case(129)
    clean[77, 1] = NAN
    everything = ref.visiting_order(cs)
    assert ref.batched_nms_fast(clean, cs, labels, 0.5).tolist() == everything
    assert batched_nms(dev(clean), dev(cs), dev(labels), 0.5).cpu().tolist() == everything


def chain_boxes(N=260):
    """scores fall with the index, so row = index.  Four boxes on one spot, each shifted by 3 in y from the one before: neighbours have IoU
    70/130 > 1/2, next-but-one neighbours 40/160.  W = 1 and Z = 3 (row block 0), Y = 70 (block 1), X = 200 (block 3): W suppresses Z, so Z
    does NOT suppress Y, so Y suppresses X.  Everything else is far away."""
    boxes = np.array([[100 * i, 0, 100 * i + 10, 10] for i in range(N)], f32)
    for i, dy in ((1, 0), (3, 3), (70, 6), (200, 9)):
        boxes[i] = [50000, dy, 50010, dy + 10]
    return boxes, (1 - np.arange(N) / 512).astype(f32)


def test_nms_chain_across_four_row_blocks():
    boxes, scores = chain_boxes()
    want = ref.nms_fast(boxes, scores, 0.5)
    assert 1 in want and 3 not in want and 70 in want and 200 not in want and len(want) == len(boxes) - 2
    without_w = ref.nms_fast(np.delete(boxes, 1, 0), np.delete(scores, 1), 0.5)        # indices above 1 move down by one
    assert 2 in without_w and 69 not in without_w and 199 in without_w                  # Z kept, Y gone, X back: every link of the chain holds
    got = nms(dev(boxes), dev(scores), 0.5).cpu().tolist()
    print(f'chain 1 -> 3 -> 70 -> 200: device keeps 70: {70 in got}, drops 3 and 200: {3 not in got and 200 not in got}; kept {len(got)} (twin {len(want)})')
    assert got == want.tolist()


def test_nms_ties_lower_index_wins():
    boxes, _, _ = ref.nms_clustered_case(260)
    scores = np.full(260, 0.5, f32)
    want = ref.nms_fast(boxes, scores, 0.5)
    assert 0 < len(want) < 260 and (np.diff(want) > 0).all() and want.max() >= 192     # index order, through every block of the four and a bit
    got = nms(dev(boxes), dev(scores), 0.5).cpu().tolist()
    print(f'260 equal scores: kept {len(got)} (twin {len(want)}), in index order: {got == sorted(got)}')
    assert got == want.tolist()


@pytest.mark.parametrize('max_keep', [1, 63, 64, 65, 128, 200, 500])
def test_nms_cut_at_max_keep(max_keep):
    rng = np.random.RandomState(3)
    boxes = np.array([[30 * (i % 20) + 0.3, 30 * (i // 20) + 0.7, 30 * (i % 20) + 20.8, 30 * (i // 20) + 18.95] for i in range(200)], f32)
    scores = rng.uniform(0.1, 1, 200).astype(f32)
    order = np.array(ref.visiting_order(scores), np.int64)
    assert len(ref.nms_fast(boxes, scores, 0.5)) == 200                                 # pairwise disjoint: only the cut drops anything
    seg = dev(np.array([0, 200], np.int32))
    kept, n_kept, flags = detector._nms_segments(dev(boxes), dev(order), None, None, seg[:1], seg[1:], 1, 256, 0.5, max_keep, flags=True)
    kept, n_kept, flags = kept.cpu().numpy(), n_kept.cpu().numpy(), flags.cpu().numpy()
    n = min(max_keep, 200)
    print(f'max_keep={max_keep}: n_kept {n_kept.tolist()} (exactly {n}), padding entries {int((kept[0, n:] == -1).sum())} of {max_keep - n}, flags set {int(flags.sum())}')
    assert kept.shape == (1, max_keep) and n_kept.tolist() == [n]
    assert kept[0, :n].tolist() == order[:n].tolist() and (kept[0, n:] == -1).all()
    assert set(np.unique(flags)) <= {0, 1} and np.flatnonzero(flags).tolist() == sorted(order[:n].tolist())


@functools.lru_cache(maxsize=None)
def case_nms_segments():
    counts = [0, 1, 64, 65, 300]
    parts = [ref.nms_clustered_case(n, seed=10 + i) for i, n in enumerate(counts)]
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    boxes, scores, labels = (np.concatenate([p[k] for p in parts]) for k in range(3))
    order = np.concatenate([s + np.array(ref.visiting_order(p[1]), np.int64) for s, p in zip(starts, parts)]).astype(np.int64)
    max_coord = np.array([p[0].max() if len(p[0]) else 0 for p in parts], f32)
    want = [s + ref.batched_nms_fast(p[0], p[1], p[2], 0.5, 48) for s, p in zip(starts, parts)]
    assert [len(w) for w in want][:2] == [0, 1] and len(want[4]) == 48                  # the cut falls in the last segment
    assert len(ref.batched_nms_fast(*parts[4], 0.5)) > 48 and all(0 < len(want[i]) < counts[i] for i in (2, 3))
    return counts, starts.astype(np.int32), boxes, labels.astype(np.int32), order, max_coord, want


@pytest.mark.parametrize('cap', [320, 4096])
def test_nms_five_segments_in_one_call(cap):
    counts, starts, boxes, labels, order, max_coord, want = case_nms_segments()
    d = dict(boxes=dev(boxes), order=dev(order), labels=dev(labels), max_coord=dev(max_coord), start=dev(starts), count=dev(np.array(counts, np.int32)))
    run = lambda lo, hi: detector._nms_segments(d['boxes'], d['order'], d['labels'], d['max_coord'][lo:hi].contiguous(), d['start'][lo:hi].contiguous(),
                                                d['count'][lo:hi].contiguous(), hi - lo, cap, 0.5, 48, flags=True)
    kept, n_kept, flags = run(0, 5)
    again = run(0, 5)
    same_bytes = all(torch.equal(a, b) for a, b in zip((kept, n_kept, flags), again))
    singles = [run(b, b + 1) for b in range(5)]
    kept_h, n_h = kept.cpu().numpy(), n_kept.cpu().numpy()
    alone = all(torch.equal(singles[b][0][0], kept[b]) and int(singles[b][1][0]) == int(n_h[b]) for b in range(5))
    print(f'cap={cap}: n_kept {n_h.tolist()} (twin {[len(w) for w in want]}), two runs equal bytes: {same_bytes}, every segment as alone: {alone}')
    assert n_h.tolist() == [len(w) for w in want]
    for b in range(5):
        assert kept_h[b, :n_h[b]].tolist() == want[b].tolist() and (kept_h[b, n_h[b]:] == -1).all()
    assert np.flatnonzero(flags.cpu().numpy()).tolist() == sorted(np.concatenate(want).tolist())
    assert same_bytes and alone


# ==== decode, gather, postprocess ===================================================================================================
def twin_flat(want):
    im = np.concatenate([np.full(len(o['scores']), b) for b, o in enumerate(want)]).astype(np.int64)
    cat = lambda k: np.concatenate([o[k] for o in want])
    return im, cat('proposal').astype(np.int64), cat('labels').astype(np.int64), cat('boxes_net').reshape(-1, 4)


def ratios_of(net_sizes, orig_sizes, im):
    net, orig = np.asarray(net_sizes, np.int64)[im], np.asarray(orig_sizes, np.int64)[im]
    rw, rh = orig[:, 1].astype(f32) / net[:, 1].astype(f32), orig[:, 0].astype(f32) / net[:, 0].astype(f32)
    return np.stack([rw, rh, rw, rh], 1).astype(f32)


def run_device(logits, reg, props, net_sizes, orig_sizes, **kw):
    args = (dev(logits), dev(reg), [dev(p) for p in props], net_sizes)
    boxes, scores, labels, im, src = postprocess_detections(*args, original_sizes=orig_sizes, return_source=True, **kw)
    boxes_net = postprocess_detections(*args, **kw)[0]
    assert boxes.dtype == torch.float32 and scores.dtype == torch.float32 and labels.dtype == im.dtype == src.dtype == torch.int64
    return dict(boxes=boxes.cpu().numpy(), boxes_net=boxes_net.cpu().numpy(), scores=scores.cpu().numpy(), labels=labels.cpu().numpy(),
                im=im.cpu().numpy(), src=src.cpu().numpy())


def check(tag, got, w_im, w_prop, w_label, w_boxes_net, logits, reg, props, net_sizes, orig_sizes):
    """ids for equality, boxes against decode64 within its bound and against the twin within 4 ulps, frame boxes bit for bit, scores within
    (C + 20) 2^-24 of the float64 softmax -> worst fraction of the decode64 bound"""
    C = logits.shape[1]
    assert got['im'].tolist() == w_im.tolist() and got['labels'].tolist() == w_label.tolist()
    assert (got['src'] // (C - 1)).tolist() == w_prop.tolist() and (got['src'] % (C - 1) + 1).tolist() == w_label.tolist()
    if len(w_im) == 0:
        print(f'{tag}: no detections on either side')
        return 0.0
    first = np.concatenate([[0], np.cumsum([len(p) for p in props])])[w_im]
    rows = first + w_prop
    s64 = ref.scores64(logits[rows]).numpy()[np.arange(len(rows)), w_label]
    err_s = np.abs(got['scores'].astype(np.float64) / s64 - 1).max()
    b64, bound = ref.decode64(reg[rows], np.concatenate(props)[rows])
    b64, bound = b64[np.arange(len(rows)), w_label], bound[np.arange(len(rows)), w_label]
    net = np.asarray(net_sizes, np.float64)[w_im]
    b64[:, 0::2] = np.clip(b64[:, 0::2], 0, net[:, 1:2])
    b64[:, 1::2] = np.clip(b64[:, 1::2], 0, net[:, 0:1])
    frac = (np.abs(got['boxes_net'].astype(np.float64) - b64) / np.maximum(bound, 1e-300)).max()
    err_b = ulps(got['boxes_net'], w_boxes_net).max()
    exact = np.array_equal(got['boxes'], got['boxes_net'] * ratios_of(net_sizes, orig_sizes, w_im))
    print(f'{tag}: D={len(rows)} boxes vs float64 {frac:.3f} of the derived bound (bound 1), vs the float32 twin {err_b:.3g} ulps (bound 4), score err '
          f'{err_s:.3g} (bound {(C + 20) * U:.3g}), frame boxes = boxes_net x own ratio bit for bit: {exact}')
    assert frac <= 1 and err_b <= 4 and err_s <= (C + 4 + 16) * U and exact
    return frac


def callable_scores(logits, thresh=0.05):
    """no float64 score within 1e-4 of the threshold: the candidate set is not a matter of rounding"""
    return int(((ref.scores64(logits)[:, 1:] - thresh).abs() < 1e-4).sum()) == 0


def strong(logits, row, label, value=9.0):
    logits[row] = -8
    logits[row, label] = value


SIZES_NET = [(200, 300), (64, 48), (50, 70), (90, 120)]                     # image 0's is the largest; image 1's is a portrait
SIZES_ORIG = [(100, 150), (128, 96), (75, 105), (45, 60)]


@functools.lru_cache(maxsize=None)
def case_per_image_sizes():
    counts, C = [70, 3, 0, 130], 4
    logits, reg, props = ref.head_case(31, counts, C, (50, 48))
    reg = reg.reshape(-1, C, 4)
    # planted: each clips at a side of ITS image; image 0's limits (300, 200) would leave right and bottom alone
    props[1][:] = [[30, 10, 60, 30], [10, 50, 30, 80], [-10, -8, 20, 20]]                # right of 48; below 64; left of and above 0
    props[3][0], props[3][1] = [100, 20, 150, 60], [20, 70, 60, 110]                     # right of 120; below 90
    for row, label in ((70, 1), (71, 2), (72, 3), (73, 1), (74, 2)):
        strong(logits, row, label, 9.0 - 0.1 * (row - 70))
        reg[row] = 0
    reg = reg.reshape(-1, 4 * C)
    assert callable_scores(logits)
    want = ref.postprocess(logits, reg, props, SIZES_NET, SIZES_ORIG)
    found = {(b, int(p), int(l)): o['boxes_net'][i] for b, o in enumerate(want) for i, (p, l) in enumerate(zip(o['proposal'], o['labels']))}
    assert found[(1, 0, 1)].tolist() == [30, 10, 48, 30] and found[(1, 1, 2)].tolist() == [10, 50, 30, 64] and found[(1, 2, 3)].tolist() == [0, 0, 20, 20]
    assert found[(3, 0, 1)].tolist() == [100, 20, 120, 60] and found[(3, 1, 2)].tolist() == [20, 70, 60, 90]
    assert len(want[2]['scores']) == 0 and all(len(want[b]['scores']) > 0 for b in (0, 1, 3))
    return logits, reg, props, want


def test_postprocess_with_per_image_sizes():
    logits, reg, props, want = case_per_image_sizes()
    got = run_device(logits, reg, props, SIZES_NET, SIZES_ORIG)
    check('per-image sizes', got, *twin_flat(want), logits, reg, props, SIZES_NET, SIZES_ORIG)
    frame = np.concatenate([o['boxes'] for o in want])
    assert ulps(got['boxes'], frame).max() <= 5                                         # and the twin's own frame boxes: 4 ulps and the product


@functools.lru_cache(maxsize=None)
def case_many_images(which):
    counts = {'singles': [1] * 130, 'gaps': [0, 2, 0, 0, 1, 70, 0]}[which]
    B, C = len(counts), 3
    logits, reg, props = ref.head_case({'singles': 41, 'gaps': 43}[which], counts, C, (37, 53))
    logits = (logits * 0.5).astype(f32)                                                 # most proposals emit: many images' atomics per wave
    net = [(37 + b % 4, 53 + b % 5) for b in range(B)]
    orig = [(24 + b % 3, 40 + b % 7) for b in range(B)]
    assert callable_scores(logits)
    want = ref.postprocess(logits, reg, props, net, orig)
    have = [len(o['scores']) > 0 for o in want]
    assert sum(have) >= 65 if which == 'singles' else have == [c > 0 for c in counts]
    return counts, logits, reg, props, net, orig, want


@pytest.mark.parametrize('which', ['singles', 'gaps'])
def test_postprocess_many_images_per_wave(which):
    counts, logits, reg, props, net, orig, want = case_many_images(which)
    got = run_device(logits, reg, props, net, orig)
    check(f'counts {which}', got, *twin_flat(want), logits, reg, props, net, orig)
    # every image alone gives the bits it gives in the batch
    first, differ = np.concatenate([[0], np.cumsum(counts)]), 0
    for b in range(len(counts)):
        rows = slice(first[b], first[b + 1])
        one = postprocess_detections(dev(logits[rows]), dev(reg[rows]), [dev(props[b])], [net[b]], [orig[b]], return_source=True)
        mine = got['im'] == b
        differ += int(not (np.array_equal(one[0].cpu().numpy(), got['boxes'][mine]) and np.array_equal(one[1].cpu().numpy(), got['scores'][mine])
                           and np.array_equal(one[2].cpu().numpy(), got['labels'][mine]) and np.array_equal(one[4].cpu().numpy(), got['src'][mine])))
    print(f'counts {which}: images whose result alone differs from the batch: {differ} of {len(counts)} (bound 0)')
    assert differ == 0


def test_postprocess_without_any_proposal():
    z = lambda *s: torch.zeros(s, device='cuda')
    out = postprocess_detections(z(0, 3), z(0, 12), [z(0, 4)] * 3, [(37, 53)] * 3, [(24, 40)] * 3, return_source=True)
    print(f'R=0, B=3: {[tuple(t.shape) for t in out]} (all empty)')
    assert [tuple(t.shape) for t in out] == [(0, 4), (0,), (0,), (0,), (0,)]
    out = postprocess_detections(z(0, 3), z(0, 12), z(0, 4), [(37, 53)] * 3, counts=[0, 0, 0])
    assert [tuple(t.shape) for t in out] == [(0, 4), (0,), (0,), (0,)]


@functools.lru_cache(maxsize=None)
def case_image_limit():
    B = detector.MAX_IMAGES
    assert B == 2047
    logits, reg, props = ref.head_case(77, [1] * B, 2, (37, 53))
    props = np.concatenate(props)
    net = [(37 + b % 5, 53 + b % 7) for b in range(B)]
    orig = [(24 + b % 3, 40 + b % 4) for b in range(B)]
    strong(logits, B - 1, 1)                                                            # the last image certainly has a detection
    assert callable_scores(logits)
    # the twin's steps 1-4 in one vectorised call; with one candidate per image NMS is the identity
    sc = ref.scores32(logits)[:, 1]
    bx = ref.decode(reg, props)[:, 1]
    nw, nh = torch.tensor([n[1] for n in net], dtype=torch.float32), torch.tensor([n[0] for n in net], dtype=torch.float32)
    zero = torch.zeros(())
    bx = torch.stack([torch.minimum(torch.maximum(bx[:, 0], zero), nw), torch.minimum(torch.maximum(bx[:, 1], zero), nh),
                      torch.minimum(torch.maximum(bx[:, 2], zero), nw), torch.minimum(torch.maximum(bx[:, 3], zero), nh)], 1)
    for b in (0, 5, 2046):
        assert torch.equal(bx[b], ref.clip(ref.decode(reg[b:b + 1], props[b:b + 1]), net[b])[0, 1])
    ok = (sc > 0.05) & ((bx[:, 2] - bx[:, 0]) >= ref.MIN_SIZE) & ((bx[:, 3] - bx[:, 1]) >= ref.MIN_SIZE)
    im = torch.nonzero(ok).reshape(-1).numpy()
    assert (im >= 1024).sum() > 100 and (im < 1024).sum() > 100 and 2046 in im.tolist()
    return logits, reg, props, net, orig, im, bx.numpy()[im]


def test_postprocess_at_2047_images():
    logits, reg, props, net, orig, im, boxes_net = case_image_limit()
    got = run_device(logits, reg, [props[b:b + 1] for b in range(len(net))], net, orig, max_candidates=64)
    check('B=2047', got, im, np.zeros(len(im), np.int64), np.ones(len(im), np.int64), boxes_net, logits, reg, [props[b:b + 1] for b in range(len(net))],
          net, orig)
    assert (got['im'] >= 1024).sum() > 100


def test_postprocess_refuses_beyond_the_key_fields(monkeypatch):
    e = lambda *s: torch.empty(s, device='cuda')
    monkeypatch.setattr(detector._lib, 'lib', boom)
    with pytest.raises(ValueError, match='2048 images exceed the limit of 2047'):
        postprocess_detections(e(2048, 2), e(2048, 8), e(2048, 4), [(37, 53)] * 2048, counts=[1] * 2048)
    with pytest.raises(ValueError, match=r'exceeds the limit of 2\^21'):
        postprocess_detections(e(2 ** 21 + 1, 2), e(2 ** 21 + 1, 8), [e(2 ** 21 + 1, 4)], [(37, 53)])
    with pytest.raises(ValueError, match='C = 4097 classes exceed the limit of 4096'):
        postprocess_detections(e(1, 4097), e(1, 4 * 4097), [e(1, 4)], [(37, 53)])


INDEX_NET, INDEX_ORIG = (480, 640), (240, 320)


@functools.lru_cache(maxsize=None)
def case_index_limit():
    R, C = 1 << 21, 2
    rng = np.random.RandomState(5)
    rows = np.unique(np.concatenate([[0, 1, R - 2, R - 1], rng.randint(2, R - 64, 84), R - 64 + rng.choice(62, 12, replace=False)]))
    assert (rows >= R - 64).sum() >= 14 and len(rows) >= 95                             # planted rows in the last wave
    logits = np.empty((R, C), f32)
    logits[:, 0], logits[:, 1] = 8, -8                                                  # background everywhere: score e^-16
    reg = np.zeros((R, 4 * C), f32)
    props = np.tile(np.array([10, 10, 30, 30], f32), (R, 1))
    for k, r in enumerate(rows):
        x, y = 40.37 * (k % 15) + 3, 40.21 * (k // 15) + 3
        props[r] = [x, y, x + 24, y + 24]
        logits[r] = [-3, rng.uniform(0, 4)]
        reg[r, 4:] = rng.uniform(-1, 1, 4)
    # two pairs of EQUAL logits at the two ends of the index range: (0, R-1) overlap with IoU 1/3 -- both kept, 0 listed first; (1, R-2) overlap
    # with IoU 5/7 -- the lower index wins, R-2 is suppressed
    for a, b, shift, logit in ((0, R - 1, 12, 5.0), (1, R - 2, 4, 4.5)):
        props[b] = props[a] + f32([shift, 0, shift, 0])
        logits[a] = logits[b] = [-3, logit]
        reg[a] = reg[b] = 0
    assert float(ref.scores32(logits[2:3])[0, 1]) < 1e-6 or 2 in rows
    sub = ref.postprocess(logits[rows], reg[rows], [props[rows]], [INDEX_NET], [INDEX_ORIG], detections_per_img=200)[0]
    src = rows[sub['proposal']]
    where = {int(s): i for i, s in enumerate(src)}
    assert where[R - 1] == where[0] + 1 and 1 in where and R - 2 not in where and len(src) >= 90
    assert len(np.unique(sub['scores'])) >= len(src) - 1                                # only the planted pair is equal
    return logits, reg, props, rows, sub, src


def test_postprocess_at_two_to_the_21_candidates():
    logits, reg, props, rows, sub, src = case_index_limit()
    R = len(logits)
    got = run_device(logits, reg, [props], [INDEX_NET], [INDEX_ORIG], detections_per_img=200)
    print(f'R=2^21: sources returned {len(got["src"])} (twin {len(src)}), the largest {got["src"].max() if len(got["src"]) else None} (2^21 - 1 = {R - 1}), '
          f'differing from the twin {int((got["src"] != src).sum()) if len(got["src"]) == len(src) else -1} (bound 0)')
    assert got['src'].tolist() == src.tolist() and got['src'].max() == R - 1
    check('R=2^21', got, np.zeros(len(src), np.int64), src, sub['labels'].astype(np.int64), sub['boxes_net'], logits, reg, [props], [INDEX_NET], [INDEX_ORIG])


def test_decode_sort_keys_hold_their_three_fields():
    """cosy_det_decode's keys against the documented packing, image << 52 | (0x7fffffff - score bits) << 21 | candidate index, rebuilt from the
    call's own scores and candidate indices: a field one bit too narrow or too wide is an unequal key.  The R = 2^21 input as three images,
    the middle one with candidate indices beyond 2^20."""
    from cosypose_amd._lib import lib, ptr
    logits, reg, props, rows, _, _ = case_index_limit()
    R, C, B, cap = len(logits), 2, 3, 256
    offsets = np.array([0, 5, R - 3, R], np.int32)
    i32 = torch.int32
    boxes, scores, labels, src = cuda((B * cap, 4)), cuda(B * cap), cuda(B * cap, i32), cuda(B * cap, i32)
    keys, counts, max_coord = cuda(B * cap, torch.int64), cuda(B, i32), cuda(B)
    ins = [dev(logits), dev(reg), dev(props), dev(offsets), dev(np.array([480, 640] * B, f32))]          # (held until the call has run)
    rc = lib().cosy_det_decode(*[ptr(t) for t in ins], R, C, B, 0.05, cap, ptr(boxes), ptr(scores), ptr(labels), ptr(src), ptr(keys), ptr(counts), ptr(max_coord), None)
    torch.cuda.synchronize()
    assert rc == 0
    n, keys, bits, src = counts.cpu().numpy(), keys.cpu().numpy(), scores.cpu().numpy().view(np.int32).astype(np.int64), src.cpu().numpy().astype(np.int64)
    image = np.array([int(((rows >= offsets[b]) & (rows < offsets[b + 1])).sum()) for b in range(B)])
    assert n.tolist() == image.tolist() and image.min() >= 1 and image.max() <= cap           # every planted row is a candidate of its image
    want = np.empty(B * cap, np.int64)
    for b in range(B):
        used = np.arange(cap) < n[b]
        at = slice(b * cap, (b + 1) * cap)
        want[at] = np.where(used, (b << 52) | ((0x7fffffff - bits[at]) << 21) | src[at], (b << 52) | ((1 << 52) - 1))
    live = np.concatenate([np.arange(cap) < n[b] for b in range(B)])
    print(f'keys of {int(live.sum())} candidates in 3 images, largest candidate index {int(src[live].max())} (2^20 = {1 << 20}): keys differing from '
          f'image << 52 | score << 21 | index {int((keys != want).sum())} of {B * cap} (bound 0)')
    assert src[live].max() >= 1 << 20
    assert np.array_equal(keys, want)
    assert sorted((src[cap:cap + n[1]] + 5).tolist()) == [int(r) for r in rows if 5 <= r < R - 3]     # candidate index = proposal in ITS image


@functools.lru_cache(maxsize=None)
def case_class_limit():
    R, C = 65, 4096
    rng = np.random.RandomState(8)
    logits = rng.uniform(-8, -6, (R, C)).astype(f32)                                    # 4094 small terms in every row's sum
    logits[:, 0] = 6.0
    steps = rng.permutation(R)
    for r in range(R):                                                                  # one class per row against the background: sigmoid(a - 6)
        logits[r, rng.randint(1, C)] = 5.5 + 0.03 * steps[r]
    logits[0, 4095] = 7.5                                                               # the last class, certainly a candidate
    _, reg, props = ref.head_case(8, [R], C, (37, 53))
    assert callable_scores(logits)
    s64 = ref.scores64(logits)[:, 1:].numpy().reshape(-1)
    s64 = np.sort(s64[s64 > 0.05])
    assert len(s64) >= R and (np.diff(s64) > 4 * (C + 20) * U * s64[1:]).all()          # the ranking is not a matter of rounding either
    want = ref.postprocess(logits, reg, props, [(37, 53)], [(24, 40)], detections_per_img=200)
    assert len(want[0]['scores']) > 30 and 4095 in want[0]['labels']
    return logits, reg, props, want


def test_postprocess_at_4096_classes():
    logits, reg, props, want = case_class_limit()
    got = run_device(logits, reg, props, [(37, 53)], [(24, 40)], detections_per_img=200)
    check('C=4096', got, *twin_flat(want), logits, reg, props, [(37, 53)], [(24, 40)])


def test_score_threshold_is_strict_at_exact_scores():
    net = [(37, 53)]
    props = np.array([[2, 3, 12, 13], [30, 20, 44, 31]], f32)
    for C, row, v in ((2, [1.5, 1.5], 0.5), (5, [-100, 2, 2, 2, 2], 0.25)):
        logits = np.tile(np.array(row, f32), (2, 1))
        reg = np.zeros((2, 4 * C), f32)
        at = postprocess_detections(dev(logits), dev(reg), [dev(props)], net, score_thresh=v)
        below = postprocess_detections(dev(logits), dev(reg), [dev(props)], net, score_thresh=float(np.nextafter(f32(v), f32(0))))
        print(f'C={C}: score_thresh={v}: {len(at[1])} detections (by hand 0); one float32 below: {len(below[1])} (by hand {2 * (C - 1)}), scores {set(below[1].cpu().tolist())}')
        assert len(at[1]) == 0
        assert len(below[1]) == 2 * (C - 1) and (below[1] == v).all()                   # identical boxes of C - 1 labels: the shift keeps them all
        assert sorted(below[2].cpu().tolist()) == sorted(list(range(1, C)) * 2)
        assert np.array_equal(below[0].cpu().numpy()[::C - 1], props)                   # zero deltas decode to the proposal, exactly


def test_small_box_threshold_is_exact():
    w = f32(0.01)
    under = np.nextafter(w, f32(0))
    logits, reg = np.array([[0, 6]] * 4, f32), np.zeros((4, 8), f32)
    # zero deltas: cx = 0 + w/2, pw = exp(0) w = w, x1 = w/2 - w/2 = 0 and x2 = w/2 + w/2 = w, all exact: the width is the proposal's
    props = np.array([[0, 5, w, 15], [0, 20, under, 30], [5, 0, 15, w], [20, 0, 30, under]], f32)
    boxes, scores, labels, im, src = postprocess_detections(dev(logits), dev(reg), [dev(props)], [(37, 53)], return_source=True)
    print(f'sides of fl32(0.01) and one float32 below, in x and in y: kept proposals {sorted(src.cpu().tolist())} (by hand [0, 2])')
    assert sorted(src.cpu().tolist()) == [0, 2]
    got = boxes.cpu().numpy()[np.argsort(src.cpu().numpy())]
    assert np.array_equal(got, props[[0, 2]])


@functools.lru_cache(maxsize=None)
def case_non_finite():
    C = 5
    logits, reg, props = ref.head_case(51, [70, 40], C, (37, 53))
    reg = reg.reshape(-1, C, 4)
    clean_l, clean_r, clean_p = logits.copy(), reg.copy(), [p.copy() for p in props]
    silent = [10, 11, 13, 14, 15, 80, 82]                                              # rows that must emit nothing at all
    for r in silent:
        clean_l[r] = -8
        clean_l[r, 0] = 8
    logits[10, 2] = NAN                                                                # a NaN logit: every score of the row is NaN
    logits[11, 3] = INF                                                                # inf - inf
    logits[12, 3] = -INF                                                               # that class scores 0, the others as with -100
    clean_l[12, 3] = -100
    reg[13], reg[14] = NAN, INF                                                        # NaN boxes; centres at infinity clip to zero width
    reg[15, :, 2:] = -INF                                                              # exp(-inf) = 0: zero size
    reg[80, :, 0] = -INF
    props[1][12] = [30, 10, 20, 25]                                                    # row 82: negative width
    reg, clean_r = reg.reshape(-1, 4 * C), clean_r.reshape(-1, 4 * C)
    assert callable_scores(clean_l) and callable_scores(np.delete(logits, [10, 11], 0))
    net, orig = [(37, 53), (40, 50)], [(24, 40), (80, 100)]
    want = ref.postprocess(logits, reg, props, net, orig)
    clean = ref.postprocess(clean_l, clean_r, clean_p, net, orig)
    for a, b in zip(want, clean):                                                      # the twin: the broken rows emit nothing, the rest is as clean
        assert all(np.array_equal(a[k], b[k]) for k in a)
    emitted = {(b, int(p)) for b, o in enumerate(want) for p in o['proposal']}
    assert not emitted & {(0, 10), (0, 11), (0, 13), (0, 14), (0, 15), (1, 10), (1, 12)} and len(emitted) > 20
    return (logits, reg, props), (clean_l, clean_r, clean_p), net, orig, want


def test_postprocess_with_non_finite_inputs():
    dirty, clean, net, orig, want = case_non_finite()
    got = run_device(*dirty, net, orig)
    check('non-finite inputs', got, *twin_flat(want), *dirty, net, orig)
    ref_run = run_device(*clean, net, orig)
    same = all(np.array_equal(got[k], ref_run[k]) for k in got)
    print(f'non-finite inputs: every array bit-identical to the run with those rows silenced: {same}')
    assert same


@functools.lru_cache(maxsize=None)
def case_bulk_ties():
    R, C = 100, 4
    rng = np.random.RandomState(13)
    logits = np.zeros((R, C), f32)                                                     # every score is exactly 1/4: 300 candidates, one score
    centre = rng.uniform(8, 30, (12, 2))[rng.randint(0, 12, R)] + rng.normal(0, 1.0, (R, 2))
    size = rng.uniform(8, 12, (R, 2))
    props = np.concatenate([centre - size / 2, centre + size / 2], 1).astype(f32)
    reg = (rng.uniform(-0.3, 0.3, (R, C, 4))).astype(f32).reshape(R, 4 * C)
    want = ref.postprocess(logits, reg, [props], [(37, 53)], [(24, 40)])
    n = len(want[0]['scores'])
    assert (want[0]['scores'] == 0.25).all() and 10 < n < 100 and len(set(want[0]['labels'].tolist())) == 3
    cand = want[0]['proposal'] * (C - 1) + want[0]['labels'] - 1
    assert (np.diff(cand) > 0).all()                                                   # equal scores: by candidate index
    return logits, reg, props, want


def test_postprocess_with_300_equal_scores():
    logits, reg, props, want = case_bulk_ties()
    got = run_device(logits, reg, [props], [(37, 53)], [(24, 40)])
    check('300 equal scores', got, *twin_flat(want), logits, reg, [props], [(37, 53)], [(24, 40)])
    again = run_device(logits, reg, [props], [(37, 53)], [(24, 40)])
    same = all(np.array_equal(got[k], again[k]) for k in got)
    print(f'300 equal scores: kept {len(got["src"])}, two runs equal bytes: {same}')
    assert same and (got['scores'] == 0.25).all()


def test_candidate_cap_boundary_and_detections_per_img():
    def case(n):
        props = np.array([[3 * (i % 16) + 0.5, 4 * (i // 16) + 0.5, 3 * (i % 16) + 2.5, 4 * (i // 16) + 3.5] for i in range(n)], f32)    # disjoint
        logits = np.stack([np.full(n, -2, f32), np.linspace(1, 3, n).astype(f32)], 1)
        return logits, np.zeros((n, 8), f32), props
    (l3, r3, p3), (l64, r64, p64), (l65, r65, p65) = case(3), case(64), case(65)
    net = [(37, 53)] * 2
    args = lambda la, ra, pa, lb, rb, pb: (dev(np.concatenate([la, lb])), dev(np.concatenate([ra, rb])), [dev(pa), dev(pb)], net)
    full = postprocess_detections(*args(l3, r3, p3, l64, r64, p64), max_candidates=64, detections_per_img=1000, return_source=True)
    one = postprocess_detections(*args(l3, r3, p3, l64, r64, p64), max_candidates=64, detections_per_img=1, return_source=True)
    print(f'64 candidates at max_candidates=64: {int((full[3] == 1).sum())} detections of image 1 (by hand 64); detections_per_img=1: sources {one[4].cpu().tolist()} (by hand [2, 63])')
    assert full[3].cpu().tolist() == [0] * 3 + [1] * 64
    assert full[4].cpu().tolist() == [2, 1, 0] + list(range(63, -1, -1))                # by descending score; disjoint boxes: all kept
    assert one[3].cpu().tolist() == [0, 1] and one[4].cpu().tolist() == [2, 63]
    with pytest.raises(ValueError, match=r'image 1 has 65 candidates above the score threshold, more than max_candidates = 64'):
        postprocess_detections(*args(l3, r3, p3, l65, r65, p65), max_candidates=64)
    assert len(postprocess_detections(*args(l3, r3, p3, l65, r65, p65), max_candidates=128)[1]) == 68


# ==== paste =========================================================================================================================
PASTE = ref.paste_edge_cases()


def paste_check(name, c, mask_th, out=None):
    """-> the device mask (D,H,W) uint8 on the host; asserts equality with paste_value64 > mask_th outside the band"""
    v64, inside = ref.paste_values64(c['logits'], c['boxes'], c['labels'], c['frame'])
    D, (H, W) = len(v64), c['frame']
    want = v64 > mask_th
    close = (np.abs(v64 - mask_th) <= 1e-5) & inside
    in_box = inside.reshape(D, -1).sum(1)
    assert (close.reshape(D, -1).sum(1) <= 1e-3 * in_box).all()                         # the reference alone stays inside the exclusion cap
    if out is None:
        out = torch.ones((D, H, W), dtype=torch.bool, device='cuda')                    # every pixel must be written
    got = paste_masks(dev(c['logits']), dev(c['boxes']), dev(c['labels']), c['frame'], mask_th, out=out)
    assert got is out
    got = got.view(torch.uint8).cpu().numpy()
    differ = ((got != 0) != want) & ~close
    print(f'{name} M={c["M"]} frame={c["frame"]} mask_th={mask_th}: in-box pixels {in_box.tolist()}, true {int(want.sum())}, in the band {int(close.sum())}; '
          f'differing pixels {int(differ.sum())} (bound 0)')
    assert set(np.unique(got)) <= {0, 1}
    assert differ.sum() == 0, np.argwhere(differ)[:10]
    return got, v64, inside


@pytest.mark.parametrize('M', [1, 2, 61, 62])
def test_paste_at_the_ends_of_M(M):
    got, v64, inside = paste_check(f'M{M}', PASTE[f'M{M}'], 0.5)
    assert inside[3].all() and inside[0].any() and got.any()


def test_paste_refuses_M_63(monkeypatch):
    monkeypatch.setattr(detector._lib, 'lib', boom)
    z = lambda *s: torch.zeros(s, device='cuda')
    with pytest.raises(ValueError, match='side 1 <= M <= 62, got C = 3, M = 63'):
        paste_masks(z(2, 3, 63, 63), z(2, 4), torch.zeros(2, dtype=torch.int64, device='cuda'), (24, 40))


@pytest.mark.parametrize('name', ['chunks', 'one_pixel_frame', 'one_row', 'one_column_wide', 'one_column_scalar'])
def test_paste_frames_at_workgroup_and_row_edges(name):
    c = PASTE[name]
    got, v64, inside = paste_check(name, c, 0.5)
    assert got.any() and not got.all()
    if name == 'chunks':
        rows = [np.flatnonzero(i.any(1))[[0, -1]].tolist() for i in inside]
        assert got[5, 127].any() and got[6, 128].any()                                  # the one-row boxes are not empty
        assert rows == [[128, 151], [98, 127], [135, 204], [3, 259], [256, 259], [127, 127], [128, 128]]      # the in-frame rows the boxes were built for


@pytest.mark.parametrize('offset', [1, 3, 15])
def test_paste_into_an_unaligned_output(offset):
    c = PASTE['alignment']
    D, (H, W) = len(c['boxes']), c['frame']
    n = D * H * W
    assert (H * W) % 16 == 0
    aligned, _, _ = paste_check('aligned', c, 0.5)
    buf = torch.ones(n + 64, dtype=torch.bool, device='cuda')
    assert buf.data_ptr() % 16 == 0
    out = buf[offset:offset + n].view(D, H, W)
    assert out.data_ptr() % 16 == offset and out.is_contiguous()
    got, _, _ = paste_check(f'{offset} bytes off', c, 0.5, out=out)
    whole = buf.view(torch.uint8).cpu().numpy()
    print(f'offset {offset}: equal to the aligned call: {np.array_equal(got, aligned)}; guard bytes changed: {int((whole[:offset] != 1).sum() + (whole[offset + n:] != 1).sum())} (bound 0)')
    assert np.array_equal(got, aligned) and aligned.any()
    assert (whole[:offset] == 1).all() and (whole[offset + n:] == 1).all()


def test_paste_degenerate_non_finite_and_clamped_boxes():
    c = PASTE['boxes']
    got, v64, inside = paste_check('boxes', c, 0.5)
    assert not got[0].any() and not got[1].any() and not got[2].any()                   # inverted in x, in y, in both: empty
    only00 = np.zeros(c['frame'], bool)
    only00[0, 0] = True
    centre = lambda d: (1 / (1 + np.exp(-c['logits'][d, c['labels'][d]].astype(np.float64))))[6:8, 6:8].mean()
    assert np.array_equal(inside[4], only00) and abs(v64[4, 0, 0] - centre(4)) < 1e-12 and np.array_equal(got[4] != 0, only00)      # all NaN: the centre value at (0, 0)
    assert inside[3].sum() == 12 and inside[3][4:16, 0].all()                           # x is NaN: column 0 of rows 4 .. 15
    assert inside[5].all() and not v64[5].any() and not got[5].any()                    # (0, 0, 2^29, 2^29): the frame sees the corner's zero ring
    assert np.array_equal(inside[7], only00)                                            # inf - inf on both axes: as the all-NaN box
    assert inside[8].all() and np.abs(v64[8] - centre(8)).max() < 1e-4 and got[8].all() # +-2^29: the centre value over the whole frame
    assert inside[9].all() and inside[10].sum() == 1 and inside[10][9, 7]               # exactly the frame; zero area at (7, 9): one pixel


def test_paste_labels_outside_the_channels():
    c = PASTE['labels']
    got, _, _ = paste_check('labels', c, 0.5)
    assert not got[0].any() and not got[1].any() and not got[3].any() and got[2].any()  # -1, C and -7 paste nothing; the plane was written
    got, _, _ = paste_check('labels', c, -0.5)
    assert got.all()                                                                    # ... the value 0, which is > -0.5


@pytest.mark.parametrize('mask_th', [-0.5, 0.0, 1.0, NAN])
def test_paste_mask_th_applies_to_every_pixel(mask_th):
    c = PASTE['mask_th']
    got, v64, inside = paste_check('mask_th', c, mask_th)
    want = {-0.5: np.ones_like(inside), 0.0: inside, 1.0: np.zeros_like(inside)}.get(mask_th, np.zeros_like(inside))   # NaN: nothing is > NaN
    assert np.array_equal(got != 0, want) and inside[:3].any() and not inside.all()


# ==== the C entry points' refusals ==================================================================================================
class Call:
    """a C entry point with a valid argument list by name; call(name=value, ...) replaces some"""

    def __init__(self, fn, outputs, **args):
        self.fn, self.outputs, self.args = fn, outputs, args

    def __call__(self, **kw):
        assert set(kw) <= set(self.args), set(kw) - set(self.args)
        return self.fn(*[kw.get(k, v) for k, v in self.args.items()])

    def refused(self, **kw):
        """-> (return code, outputs untouched) of a call that must be refused"""
        for t in self.outputs:
            t.fill_(7)
        rc = self(**kw)
        torch.cuda.synchronize()
        return rc, all(bool((t == 7).all()) for t in self.outputs)

    def check(self, name, bads, noops):
        for t in self.outputs:
            t.fill_(7)
        assert self() == 0
        torch.cuda.synchronize()
        assert not all(bool((t == 7).all()) for t in self.outputs)                      # the valid call does write
        wrong = []
        for bad in bads:
            rc, untouched = self.refused(**bad)
            if rc != -1 or not untouched:
                wrong.append((bad, rc, untouched))
        print(f'{name}: {len(bads)} violations, not refused with -1 and untouched outputs: {wrong} (bound: none)')
        assert not wrong
        for noop in noops:
            assert self(**noop) == 0, noop
        torch.cuda.synchronize()


def cuda(shape, dtype=torch.float32, fill=0):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), fill, dtype=dtype, device='cuda')


def nulls(*names):
    return {n: None for n in names}


def test_c_abi_det_decode_refusals():
    from cosypose_amd._lib import lib, ptr
    B, R, C, cap = 2, 6, 3, 64
    i32, i64 = torch.int32, torch.int64
    logits, reg, props = cuda((R, C)), cuda((R, 4 * C)), dev(np.tile(np.array([2, 3, 20, 25], f32), (R, 1)))
    offsets, net = dev(np.array([0, 3, 6], np.int32)), dev(np.array([37, 53, 37, 53], f32))
    outs = [cuda((B * cap, 4)), cuda(B * cap), cuda(B * cap, i32), cuda(B * cap, i32), cuda(B * cap, i64), cuda(B, i32), cuda(B)]
    call = Call(lib().cosy_det_decode, outs, logits=ptr(logits), reg=ptr(reg), props=ptr(props), offsets=ptr(offsets), net=ptr(net), R=R, C=C, B=B,
                th=0.05, cap=cap, boxes=ptr(outs[0]), scores=ptr(outs[1]), labels=ptr(outs[2]), src=ptr(outs[3]), keys=ptr(outs[4]),
                counts=ptr(outs[5]), max_coord=ptr(outs[6]), s=None)
    pointers = ['logits', 'reg', 'props', 'offsets', 'net', 'boxes', 'scores', 'labels', 'src', 'keys', 'counts', 'max_coord']
    bads = [dict(R=-1), dict(B=-1), dict(C=1), dict(C=4097), dict(B=2048), dict(cap=0), dict(cap=100), dict(cap=16384 + 64), dict(cap=-64),
            dict(R=2 ** 21 + 1, C=2), dict(R=2 ** 19 + 1, C=5), dict(th=-0.1), dict(th=NAN)] + [{p: None} for p in pointers]
    inputs = ['logits', 'reg', 'props', 'offsets', 'net', 'boxes', 'scores', 'labels', 'src']
    call.check('cosy_det_decode', bads, [dict(B=0, R=0, **nulls(*pointers)), dict(R=0, **nulls(*inputs))])
    assert outs[5].cpu().tolist() == [0, 0]                                             # R = 0: the initialisation alone ran


def nms_call_tensors():
    N, cap = 70, 128
    boxes, scores, labels = ref.nms_clustered_case(N)
    order = np.array(ref.visiting_order(scores), np.int64)
    return N, cap, dev(boxes), dev(order), dev(labels.astype(np.int32)), dev(np.array([boxes.max()], f32)), dev(np.array([0], np.int32)), dev(np.array([N], np.int32))


NMS_COMMON_BADS = [dict(B=-1), dict(N=-1), dict(B=65536), dict(cap=0), dict(cap=100), dict(cap=16384 + 64), dict(start=None), dict(count=None)]


def test_c_abi_nms_mask_refusals():
    from cosypose_amd._lib import lib, ptr
    N, cap, boxes, order, labels, max_coord, start, count = nms_call_tensors()
    mask = cuda(cap * (cap // 64) + 1, torch.int64)
    call = Call(lib().cosy_nms_mask, [mask], boxes=ptr(boxes), order=ptr(order), labels=ptr(labels), max_coord=ptr(max_coord), start=ptr(start),
                count=ptr(count), B=1, N=N, cap=cap, thr=0.5, mask=ptr(mask), s=None)
    bads = NMS_COMMON_BADS + [dict(max_coord=None), dict(boxes=None), dict(mask=None), dict(mask=ptr(mask) + 4)]
    everything = nulls('boxes', 'order', 'labels', 'max_coord', 'start', 'count', 'mask')
    call.check('cosy_nms_mask', bads, [dict(B=0, **everything), dict(N=0, boxes=None, order=None, labels=None, max_coord=None, mask=None),
                                       dict(labels=None, max_coord=None), dict(order=None)])


def test_c_abi_nms_scan_refusals():
    from cosypose_amd._lib import lib, ptr
    N, cap, boxes, order, labels, max_coord, start, count = nms_call_tensors()
    mask = cuda(cap * (cap // 64) + 1, torch.int64)
    assert lib().cosy_nms_mask(ptr(boxes), ptr(order), None, None, ptr(start), ptr(count), 1, N, cap, 0.5, ptr(mask), None) == 0
    outs = [cuda((1, 10), torch.int32), cuda(1, torch.int32), cuda(N, torch.uint8)]
    call = Call(lib().cosy_nms_scan, outs, mask=ptr(mask), order=ptr(order), start=ptr(start), count=ptr(count), B=1, N=N, cap=cap, max_keep=10,
                kept=ptr(outs[0]), n_kept=ptr(outs[1]), flags=ptr(outs[2]), s=None)
    bads = NMS_COMMON_BADS + [dict(max_keep=-1), dict(n_kept=None), dict(kept=None), dict(mask=None), dict(mask=ptr(mask) + 4)]
    everything = nulls('mask', 'order', 'start', 'count', 'kept', 'n_kept', 'flags')
    call.check('cosy_nms_scan', bads, [dict(B=0, **everything), dict(flags=None), dict(order=None), dict(max_keep=0, kept=None)])


def test_c_abi_det_gather_refusals():
    from cosypose_amd._lib import lib, ptr
    B, cap, keep = 2, 64, 3
    i32 = torch.int32
    kept, n_kept, counts = dev(np.array([[5, 2, -1], [64, -1, -1]], np.int32)), dev(np.array([2, 1], np.int32)), dev(np.array([9, 4], np.int32))
    cb, cs, cl, csrc, ratios = cuda((B * cap, 4), fill=1), cuda(B * cap, fill=0.5), cuda(B * cap, i32, 2), cuda(B * cap, i32, 3), cuda((B, 2), fill=1)
    outs = [cuda((B * keep, 4)), cuda((B * keep, 4)), cuda(B * keep, i32), cuda(2 * B + 2 * B * keep, i32)]
    call = Call(lib().cosy_det_gather, outs, kept=ptr(kept), n_kept=ptr(n_kept), counts=ptr(counts), cb=ptr(cb), cs=ptr(cs), cl=ptr(cl), csrc=ptr(csrc),
                ratios=ptr(ratios), B=B, cap=cap, max_keep=keep, boxes_net=ptr(outs[0]), boxes_frame=ptr(outs[1]), src=ptr(outs[2]), packed=ptr(outs[3]),
                s=None)
    pointers = ['kept', 'n_kept', 'counts', 'cb', 'cs', 'cl', 'csrc', 'ratios', 'boxes_net', 'boxes_frame', 'src', 'packed']
    bads = [dict(B=-1), dict(B=2048), dict(max_keep=-1), dict(cap=63), dict(cap=16385), dict(B=2047, max_keep=1 << 20)] + [{p: None} for p in pointers]
    call.check('cosy_det_gather', bads, [dict(B=0, **nulls(*pointers)),
                                         dict(max_keep=0, **nulls('kept', 'cb', 'cs', 'cl', 'csrc', 'boxes_net', 'boxes_frame', 'src'))])
    assert call() == 0
    packed = outs[3].cpu().tolist()
    assert packed[:4] == [9, 4, 2, 1] and packed[4:10] == [2, 2, -1, 2, -1, -1]         # counts, kept counts, labels with -1 on the padding


def test_c_abi_paste_masks_refusals():
    from cosypose_amd._lib import lib, ptr
    D, C, M, H, W = 2, 3, 4, 8, 16
    logits, boxes, labels = cuda((D, C, M, M), fill=2), dev(np.array([[1, 1, 9, 6], [4, 2, 14, 7]], f32)), cuda(D, torch.int32, 1)
    out = cuda((D, H, W), torch.uint8)
    call = Call(lib().cosy_paste_masks, [out], logits=ptr(logits), boxes=ptr(boxes), labels=ptr(labels), D=D, C=C, M=M, H=H, W=W, th=0.5, out=ptr(out), s=None)
    bads = [dict(D=-1), dict(C=0), dict(H=0), dict(W=0), dict(H=-3), dict(M=0), dict(M=63), dict(D=65536), dict(H=1 << 15, W=1 << 15),
            dict(logits=None), dict(boxes=None), dict(labels=None), dict(out=None)]
    call.check('cosy_paste_masks', bads, [dict(D=0, **nulls('logits', 'boxes', 'labels', 'out'))])
