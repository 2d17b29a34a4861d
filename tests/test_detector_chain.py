"""One whole training step of the detector on the GPU -- Detector.losses(...) and the backward of the sum of the five losses -- against an
independent derivative: tests/detector_chain_ref.py, plain torch in float64 on the CPU, every gradient torch.autograd's (DESIGN.md section 31;
test_detector_chain_host.py guards the reference itself).

The discrete and the detached quantities (the transformed images and targets, the RPN's matches and samples, the sampled RoIs with their labels,
matches and levels) are taken from the device run that is checked; everything else the reference computes itself.  Yardsticks, both computed in
the test from the reference alone:
  float32: e32 = the largest relative error of the reference's own float32 CPU replica against float64, over the parameters (and, each on its own,
    over the gradients retained at the five maps and over the five losses).  The device must stay within 4 x e32 for every parameter, every map and
    every loss: both are float32 chains of the same depth that differ in summation order only.
  bfloat16 trunk: s = the largest relative change that rounding at section 30's storage points makes in the float64 reference.  The device must stay
    within 2 x s for every parameter and map.
Cases (detector_chain_case.py; check_reach asserts on the device's own decisions what each was chosen to reach): small, two-levels, four-levels (one
frame, RoIs on all four maps of both paths) and mixed (three frames of three sizes with 1, 3 and 5 ground truths, a tiny and a full-frame box, an
all-zero and an all-one mask).  Every test prints its measured ratios before it asserts.

The last test holds the decisions themselves, which the derivative check takes as given, to their CPU twins fed the device's own upstream values."""
import sys

import numpy as np
import pytest
import torch

import detector_chain_case as cc
import detector_chain_ref as cr
import detpost_ref as post
import detpre_ref as pre
import dettrain_ref as tr
import dettrunk_case as tc
import cosypose_amd.detector_input                                            # noqa: F401 (the module, patched below through sys.modules)
from cosypose_amd import Detector, detector_rpn, detector_train as dt
from cosypose_amd.detector_trunk import ANCHOR_SIZES, ASPECT_RATIOS
from test_detector_rpn import check_proposals, post_ulps

pytestmark = pytest.mark.gpu
FACTOR_F32, FACTOR_BF16 = 4, 2


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def detector(case, **kw):
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in tc.detector_weights().items()}
    return Detector.from_state_dict(sd, tc.E2E_LABELS, input_resize=cc.CASES[case]['resize'], trainable=True, **kw)


def device_step(det, case, monkeypatch):
    """one losses() + backward on the device with its decisions recorded -> losses, parameter gradients, map gradients, the reference's inputs.
    The wrappers change no launch of the step: rpn_loss returns what it computed anyway, the levels come from a second RoIAlign call afterwards."""
    rec = {}
    di = sys.modules['cosypose_amd.detector_input']
    real = dict(features=di._feature_list, losses=dt.detector_losses, rpn=dt.rpn_loss, samples=dt.roi_training_samples)

    def features(backbone, images):
        rec['images'] = images
        rec['maps'] = real['features'](backbone, images)
        for m in rec['maps']:
            m.retain_grad()
        return rec['maps']

    def losses(maps, rpn_head, box_head, mask_head, targets, net_sizes, padded_size, **kw):
        rec.update(targets=targets, net_sizes=[tuple(int(v) for v in s) for s in net_sizes], padded_size=tuple(int(v) for v in padded_size))
        return real['losses'](maps, rpn_head, box_head, mask_head, targets, net_sizes, padded_size, **kw)

    def rpn(objectness, deltas, targets, net_sizes, padded_size, sizes, aspect_ratios, keys, *rest, **kw):
        rec['rpn_in'] = dict(objectness=[o.detach() for o in objectness], deltas=[d.detach() for d in deltas], net_sizes=net_sizes, padded_size=padded_size,
                             sizes=sizes, aspect_ratios=aspect_ratios, keys=keys)
        *two, rec['rpn'] = real['rpn'](objectness, deltas, targets, net_sizes, padded_size, sizes, aspect_ratios, keys, *rest, return_samples=True, **kw)
        return tuple(two)

    def samples(proposals, counts, targets, keys, *rest, **kw):
        rec['smp_in'] = dict(proposals=proposals, counts=counts, keys=keys)
        rec['smp'] = real['samples'](proposals, counts, targets, keys, *rest, **kw)
        return rec['smp']
    frames = [dev(f) for f in cc.frames(case)]
    targets = [{k: dev(v) for k, v in t.items()} for t in cc.targets(case)]
    k = cc.keys(case, cc.n_anchors(cc.padded_size(case)))
    det.zero_grad()
    with monkeypatch.context() as m:
        m.setattr(di, '_feature_list', features), m.setattr(dt, 'detector_losses', losses)
        m.setattr(dt, 'rpn_loss', rpn), m.setattr(dt, 'roi_training_samples', samples)
        out = det.losses(frames, targets, keys={name: dev(v) for name, v in k.items()})
    sum(out.values()).backward()
    torch.cuda.synchronize()
    smp, maps = rec['smp'], rec['maps']
    with torch.no_grad():
        roi_maps = [f.detach() for f in maps[:4]]
        _, roi_levels = detector_rpn.multiscale_roi_align(roi_maps, smp['boxes'], rec['net_sizes'], 7, 2, counts=smp['counts'], return_levels=True)
        _, pos_levels = detector_rpn.multiscale_roi_align(roi_maps, smp['pos_boxes'], rec['net_sizes'], 14, 2, counts=smp['pos_counts'], return_levels=True)
    matched, samp_idx, samp_count = rec['rpn']
    cpu = lambda t: t.detach().cpu()
    inp = dict(images=cpu(rec['images']), net_sizes=rec['net_sizes'], padded_size=rec['padded_size'],
               gt_boxes=[cpu(t['boxes']) for t in rec['targets']], gt_labels=[cpu(t['labels']) for t in rec['targets']],
               gt_masks=[cpu(t['masks']) for t in rec['targets']],
               anchors=detector_rpn.rpn_anchors([tuple(f.shape[2:]) for f in maps], rec['padded_size'], ANCHOR_SIZES, ASPECT_RATIOS),
               rpn_matched=cpu(matched), rpn_samp_idx=cpu(samp_idx), rpn_samp_count=cpu(samp_count),
               roi_boxes=cpu(smp['boxes']), roi_labels=cpu(smp['labels']), roi_matched=cpu(smp['matched_idxs']), roi_counts=cpu(smp['counts']),
               roi_levels=cpu(roi_levels), pos_boxes=cpu(smp['pos_boxes']), pos_labels=cpu(smp['pos_labels']), pos_matched=cpu(smp['pos_matched_idxs']),
               pos_counts=cpu(smp['pos_counts']), pos_levels=cpu(pos_levels))
    # what the two wrapped stages were handed and what the sampler wrote beside the reference's inputs: the seam test's material, still on the device
    inp['seams'] = dict(rpn=rec['rpn_in'], samples=rec['smp_in'], smp=smp)
    grads = {name: cpu(p.grad).clone() for name, p in det.named_parameters() if p.grad is not None}
    return {name: cpu(v) for name, v in out.items()}, grads, [None if f.grad is None else cpu(f.grad).clone() for f in maps], inp


def rel(got, want):
    got, want = got.double(), want.double()
    if not float(want.norm()):
        return 0.0 if not float(got.norm()) else float('inf')
    return float((got - want).norm() / want.norm())


def gradient_ratios(got, want):
    """(parameter gradients, map gradients) twice -> {name: || got - want || / || want ||}, the five maps under 'map 0' .. 'map pool'"""
    (pg, mg), (pw, mw) = got, want
    assert set(pg) == set(pw), ('the parameters that hold a gradient', sorted(set(pg) ^ set(pw)))
    assert [g is None for g in mg] == [w is None for w in mw] == [False] * 5
    out = {name: rel(pg[name], pw[name]) for name in pw}
    out.update({f'map {level}': rel(g, w) for level, g, w in zip(('0', '1', '2', '3', 'pool'), mg, mw)})
    return out


def loss_ratios(got, want):
    assert tuple(got) == tuple(want) == cr.LOSS_KEYS
    return {k: abs(float(got[k]) - float(want[k])) / abs(float(want[k])) for k in want}


CASES = [('small', 2), ('small', cc.N_STAGES + 1), ('two-levels', 2), ('four-levels', 2), ('mixed', 2), ('mixed', cc.N_STAGES + 1)]
BF16_CASES = ['small', 'four-levels', 'mixed']


@pytest.mark.parametrize('case,train_from_stage', CASES, ids=[f'{c}-from-stage-{s}' for c, s in CASES])
def test_a_training_step_meets_float64_autograd(case, train_from_stage, monkeypatch):
    det = detector(case, train_from_stage=train_from_stage)
    losses, grads, map_grads, inp = device_step(det, case, monkeypatch)
    sd = tc.detector_weights()
    chain64 = cr.Chain(sd, train_from_stage)
    l64, g64, m64 = chain64.step(inp)
    l32, g32, m32 = cr.Chain(sd, train_from_stage, dtype=torch.float32).step(inp)
    cc.check_reach(case, inp, chain64.kinks)                                     # the case is what it was chosen to be, on the device's own decisions
    # the set of parameters that hold a gradient: the reference's own, by its train_from_stage
    assert set(grads) == set(g64) == {k for k, _ in det.named_parameters()}
    assert any('body.layer2.' in k for k in grads) == (train_from_stage == 2) and not any('body.layer1.' in k or 'body.conv1' in k for k in grads)
    # losses
    e32_loss = max(loss_ratios(l32, l64).values())
    r_loss = loss_ratios(losses, l64)
    for k in cr.LOSS_KEYS:
        print(f'  {k}: device {float(losses[k]):.9g}, float64 {float(l64[k]):.12g}, relative error {r_loss[k]:.3e}')
    print(f'  losses: e32 = {e32_loss:.3e}, largest device error {max(r_loss.values()):.3e} = {max(r_loss.values()) / e32_loss:.2f} x e32 (bound: {FACTOR_F32})')
    # gradients
    r32, r_dev = gradient_ratios((g32, m32), (g64, m64)), gradient_ratios((grads, map_grads), (g64, m64))
    late = {}
    for what, own in (('parameters', lambda k: not k.startswith('map ')), ('maps', lambda k: k.startswith('map '))):     # each against its own replica's error
        e32 = max(v for k, v in r32.items() if own(k))
        worst = max((k for k in r_dev if own(k)), key=r_dev.get)
        print(f'  gradients of the {what}: e32 = {e32:.3e}, largest r_dev = {r_dev[worst]:.3e} at {worst} = {r_dev[worst] / e32:.2f} x e32 (bound: {FACTOR_F32})')
        late.update({k: (v, e32) for k, v in r_dev.items() if own(k) and not v <= FACTOR_F32 * e32})
    assert all(v <= FACTOR_F32 * e32_loss for v in r_loss.values()), r_loss
    assert not late, late
    # a second run gives equal bits
    losses2, grads2, map_grads2, _ = device_step(det, case, monkeypatch)
    assert all(torch.equal(losses[k], losses2[k]) for k in losses) and all(torch.equal(grads[k], grads2[k]) for k in grads)
    assert all(torch.equal(a, b) for a, b in zip(map_grads, map_grads2))


@pytest.mark.parametrize('case', BF16_CASES)
def test_a_training_step_with_the_bfloat16_trunk_stays_within_twice_the_storage_effect(case, monkeypatch):
    det = detector(case, train_dtype=torch.bfloat16)
    losses, grads, map_grads, inp = device_step(det, case, monkeypatch)               # the decisions of THIS run
    sd = tc.detector_weights()
    chain64 = cr.Chain(sd)
    l64, g64, m64 = chain64.step(inp)
    cc.check_reach(case, inp, chain64.kinks)
    ls, gs, ms = cr.Chain(sd, storage='bfloat16').step(inp)
    s, r_dev = gradient_ratios((gs, ms), (g64, m64)), gradient_ratios((grads, map_grads), (g64, m64))
    s_max = max(v for k, v in s.items() if not k.startswith('map '))
    worst = max(r_dev, key=r_dev.get)
    r_loss, s_loss = loss_ratios(losses, l64), loss_ratios(ls, l64)
    print(f'bfloat16 trunk on {case}: largest storage effect s = {s_max:.3e} (at {max(s, key=s.get)}), largest r_dev = {r_dev[worst]:.3e} at {worst} = '
          f'{r_dev[worst] / s_max:.2f} x s (bound: {FACTOR_BF16}); losses: device {max(r_loss.values()):.3e}, storage emulation {max(s_loss.values()):.3e}')
    assert set(grads) == set(g64) and all(g.dtype == torch.float32 for g in grads.values())
    late = {k: v for k, v in r_dev.items() if not v <= FACTOR_BF16 * s_max}
    assert s_max > 0 and not late, late
    losses2, grads2, map_grads2, _ = device_step(det, case, monkeypatch)             # a second run gives equal bits
    assert all(torch.equal(losses[k], losses2[k]) for k in losses) and all(torch.equal(grads[k], grads2[k]) for k in grads)
    assert all(torch.equal(a, b) for a, b in zip(map_grads, map_grads2))


# ---- the decisions at the seams ------------------------------------------------------------------------------------------------------------------
def explain_kept_difference(b, got_src, got_boxes, want, everything, top_n, nms_thresh=0.7, min_size=1e-3):
    """A kept list of image b differs from the twin's (the device's expf and NumPy's exp may differ in the last bit of a decoded box).  Every
    candidate in the symmetric difference must itself take part in a decision within 4 float32 ulps of its threshold: an NMS IoU at 0.7 with a
    candidate of its level, a side at min_size, or a score tie at the cut.  `everything`: the twin's decode of every candidate, no filter.
    Prints each with both values -> the candidates that no such decision explains."""
    f32 = np.float32
    near = lambda v, t: np.abs(np.asarray(v, np.float64) - float(f32(t))) <= 4 * float(np.spacing(f32(t)))
    row = {int(s): i for i, s in enumerate(everything['src'])}
    shifted = post.shifted_np(everything['boxes'], everything['levels'])
    cut = [float(scores[top_n - 1]) for scores in (want['scores'],) if len(scores) >= top_n]
    unexplained = []
    for s in sorted(set(got_src.tolist()) ^ set(want['src'].tolist())):
        i = row[s]
        box, where = everything['boxes'][i], 'the device' if s in got_src else 'the twin'
        with np.errstate(all='ignore'):
            ious = post.iou_rows_np(shifted[i], shifted)
        ious[i] = 0
        sides = (box[2] - box[0], box[3] - box[1])
        reasons = [f'IoU {float(v):.9g} with candidate {int(everything["src"][j])} against {float(f32(nms_thresh)):.9g}' for j, v in enumerate(ious) if near(v, nms_thresh)]
        reasons += [f'side {float(v):.9g} against {float(f32(min_size)):.9g}' for v in sides if near(v, min_size)]
        reasons += [f'score {float(everything["scores"][i]):.9g} tied at the cut' for c in cut if float(everything['scores'][i]) == c]
        device_box = got_boxes[got_src.tolist().index(s)].tolist() if s in got_src else None
        print(f'  image {b}: candidate {s} kept by {where} only; the twin\'s box {box.tolist()}, the device\'s {device_box}: {reasons or "NO decision within 4 ulps"}')
        if not reasons:
            unexplained.append(s)
    return unexplained


@pytest.mark.parametrize('case', list(cc.CASES))
def test_the_decisions_of_a_training_step_are_the_twins(case, monkeypatch):
    """Detector.losses at full scale (five levels, 15 anchors per cell, 2000 proposals, the real heads): every discrete decision of the step
    against its CPU twin fed the DEVICE's own upstream values -- the RPN's match and sample, the proposals, the RoI sampler's rows, the levels."""
    det = detector(case)
    _, _, _, inp = device_step(det, case, monkeypatch)
    seams, B = inp['seams'], len(inp['net_sizes'])
    host = lambda t: t.detach().cpu().numpy()
    rpn_in, smp_in, smp = seams['rpn'], seams['samples'], {k: host(v) for k, v in seams['smp'].items()}
    obj, dl = [host(o) for o in rpn_in['objectness']], [host(d) for d in rpn_in['deltas']]
    nets, pad = inp['net_sizes'], inp['padded_size']
    assert [tuple(int(v) for v in s) for s in rpn_in['net_sizes']] == nets and tuple(int(v) for v in rpn_in['padded_size']) == pad
    sizes, ratios = tuple(tuple(s) for s in rpn_in['sizes']), tuple(rpn_in['aspect_ratios'])
    assert (sizes, ratios) == (cc.SIZES, cc.RATIOS)
    gt, labels = [g.numpy() for g in inp['gt_boxes']], [l.numpy() for l in inp['gt_labels']]
    G_max = max(len(g) for g in gt)
    keys = cc.keys(case, cc.n_anchors(pad))
    assert np.array_equal(host(rpn_in['keys']), keys['rpn']) and np.array_equal(host(smp_in['keys']), keys['roi'])

    # the RPN's match and sample
    want = tr.rpn_loss(obj, dl, gt, pad, sizes, ratios, keys['rpn'], cc.RPN_BATCH)
    matched, samp_idx, samp_count = inp['rpn_matched'].numpy(), inp['rpn_samp_idx'].numpy(), inp['rpn_samp_count'].numpy()
    print(f'{case}: RPN samples {samp_count.tolist()}, of them positive {[int((want["matched"][b][s] >= 0).sum()) for b, s in enumerate(want["sampled"])]}, '
          f'anchors matched {[int((m >= 0).sum()) for m in want["matched"]]} of {matched.shape[1]}')
    assert matched.shape == want['matched'].shape and np.array_equal(matched, want['matched'])
    for b, s in enumerate(want['sampled']):
        assert samp_count[b] == len(s) and samp_idx[b, :len(s)].tolist() == s.tolist() and (samp_idx[b, len(s):] == -1).all()
        assert 0 < int((want['matched'][b][s] >= 0).sum()) < len(s)

    # the proposals: a second call on the recorded head outputs returns the sources too, and the rows the step used
    got = detector_rpn.rpn_proposals(rpn_in['objectness'], rpn_in['deltas'], nets, pad, ANCHOR_SIZES, ASPECT_RATIOS, cc.TOP_N, cc.TOP_N, return_source=True)
    assert torch.equal(got[0], smp_in['proposals']) and torch.equal(got[1], smp_in['counts'])
    want = pre.proposals(obj, dl, nets, pad, sizes, ratios, pre_nms_top_n=cc.TOP_N, post_nms_top_n=cc.TOP_N)
    props, counts, src = host(got[0]), host(got[1]), host(got[4])
    kept = [src[b * cc.TOP_N:b * cc.TOP_N + int(counts[b])] for b in range(B)]
    differ = [b for b in range(B) if kept[b].tolist() != want[b]['src'].tolist()]
    print(f'{case}: proposals kept {counts.tolist()} of {[len(w["candidates"]) for w in want]} candidates; images whose kept list differs from the twin\'s: {differ}')
    if not differ:
        check_proposals(obj, dl, nets, got, want, cc.TOP_N)                        # equal counts, kept lists, scores and levels; boxes within 4 ulps
    else:
        everything = pre.proposals(obj, dl, nets, pad, sizes, ratios, pre_nms_top_n=cc.TOP_N, post_nms_top_n=10 ** 9, nms_thresh=float('inf'), min_size=0.0)
        unexplained = {b: explain_kept_difference(b, kept[b], props[b * cc.TOP_N:b * cc.TOP_N + int(counts[b])], want[b], everything[b], cc.TOP_N)
                       for b in differ}
        assert not any(unexplained.values()), unexplained
        for b in set(range(B)) - set(differ):
            assert float(post_ulps(props[b * cc.TOP_N:b * cc.TOP_N + len(kept[b])], want[b]['boxes']).max()) <= 4

    # the RoI sampler on the device's proposals
    assert smp['boxes'].shape == (B * cc.ROI_BATCH, 4) and smp['pos_boxes'].shape == (B * cc.ROI_POSITIVES, 4)
    for b in range(B):
        want = tr.roi_samples(props[b * cc.TOP_N:b * cc.TOP_N + int(counts[b])], gt[b], labels[b], keys['roi'][b], cc.TOP_N, G_max, cc.ROI_BATCH)
        n, k = len(want['idx']), len(want['pos_idx'])
        assert (int(smp['counts'][b]), int(smp['pos_counts'][b])) == (n, k)
        rows = slice(b * cc.ROI_BATCH, b * cc.ROI_BATCH + n)
        assert np.array_equal(smp['boxes'][rows], want['boxes']) and np.array_equal(smp['labels'][rows], want['labels'])
        assert np.array_equal(smp['matched_idxs'][rows], want['matched'])
        err = np.abs(smp['regression_targets'][rows].astype(np.float64) - want['targets64'])
        print(f'  image {b}: {n} sampled RoIs, {k} positives; regression targets: largest error / the twin\'s bound = '
              f'{float((err / np.maximum(want["target_bounds"], 1e-300)).max()):.3f} (bound: 1)')
        assert np.isfinite(err).all() and (err <= want['target_bounds']).all()
        padding = slice(b * cc.ROI_BATCH + n, (b + 1) * cc.ROI_BATCH)
        assert not smp['boxes'][padding].any() and (smp['labels'][padding] == -1).all() and not smp['regression_targets'][padding].any()
        pos = slice(b * cc.ROI_POSITIVES, b * cc.ROI_POSITIVES + k)
        assert np.array_equal(smp['pos_boxes'][pos], want['pos_boxes']) and np.array_equal(smp['pos_labels'][pos], want['pos_labels'])
        assert np.array_equal(smp['pos_matched_idxs'][pos], want['pos_matched'])
        assert (smp['pos_labels'][b * cc.ROI_POSITIVES + k:(b + 1) * cc.ROI_POSITIVES] == -1).all()

    # the levels of both paths
    for boxes, levels, cnt in (('roi_boxes', 'roi_levels', 'roi_counts'), ('pos_boxes', 'pos_levels', 'pos_counts')):
        for b, (bx, lv) in enumerate(zip(cc.real_rows(inp, boxes, cnt), cc.real_rows(inp, levels, cnt))):
            assert np.array_equal(lv.numpy(), pre.map_levels(bx.numpy(), 2, 5)), (levels, b)
