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
    within 2 x s for every parameter.
Every test prints its measured ratios before it asserts."""
import sys

import numpy as np
import pytest
import torch

import detector_chain_case as cc
import detector_chain_ref as cr
import dettrunk_case as tc
import cosypose_amd.detector_input                                            # noqa: F401 (the module, patched below through sys.modules)
from cosypose_amd import Detector, detector_rpn, detector_train as dt
from cosypose_amd.detector_trunk import ANCHOR_SIZES, ASPECT_RATIOS

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

    def rpn(*args, **kw):
        *two, rec['rpn'] = real['rpn'](*args, return_samples=True, **kw)
        return tuple(two)

    def samples(*args, **kw):
        rec['smp'] = real['samples'](*args, **kw)
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


def real_rows(inp, key, counts):
    per = int(inp[key].shape[0]) // len(inp['net_sizes'])
    return [inp[key][b * per:b * per + int(c)] for b, c in enumerate(inp[counts])]


CASES = [('small', 2), ('small', cc.N_STAGES + 1), ('two-levels', 2)]


@pytest.mark.parametrize('case,train_from_stage', CASES, ids=[f'{c}-from-stage-{s}' for c, s in CASES])
def test_a_training_step_meets_float64_autograd(case, train_from_stage, monkeypatch):
    det = detector(case, train_from_stage=train_from_stage)
    losses, grads, map_grads, inp = device_step(det, case, monkeypatch)
    sd = tc.detector_weights()
    l64, g64, m64 = cr.Chain(sd, train_from_stage).step(inp)
    l32, g32, m32 = cr.Chain(sd, train_from_stage, dtype=torch.float32).step(inp)
    # the case is what it was chosen to be, on the device's own decisions
    positives, backgrounds = [int(c) for c in inp['pos_counts']], [int((l == 0).sum()) for l in real_rows(inp, 'roi_labels', 'roi_counts')]
    box_levels, mask_levels = (sorted(set(torch.cat(real_rows(inp, k, c)).tolist())) for k, c in (('roi_levels', 'roi_counts'), ('pos_levels', 'pos_counts')))
    print(f'{case}: images {tuple(inp["images"].shape)}, sampled RoIs {[int(c) for c in inp["roi_counts"]]}, positives {positives}, background rows '
          f'{backgrounds}, levels of the box path {box_levels}, of the mask path {mask_levels}')
    assert min(positives) >= 2 and min(backgrounds) >= 1
    if case == 'two-levels':
        assert len(box_levels) >= 2 and len(mask_levels) >= 2 and inp['padded_size'] == (160, 224)
        assert all(float(min(g[0, 2] - g[0, 0], g[0, 3] - g[0, 1])) > 130 for g in inp['gt_boxes'])
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


def test_a_training_step_with_the_bfloat16_trunk_stays_within_twice_the_storage_effect(monkeypatch):
    case = 'small'
    det = detector(case, train_dtype=torch.bfloat16)
    losses, grads, map_grads, inp = device_step(det, case, monkeypatch)               # the decisions of THIS run
    sd = tc.detector_weights()
    l64, g64, m64 = cr.Chain(sd).step(inp)
    ls, gs, ms = cr.Chain(sd, storage='bfloat16').step(inp)
    s, r_dev = gradient_ratios((gs, ms), (g64, m64)), gradient_ratios((grads, map_grads), (g64, m64))
    s_max = max(v for k, v in s.items() if not k.startswith('map '))
    worst = max(r_dev, key=r_dev.get)
    r_loss, s_loss = loss_ratios(losses, l64), loss_ratios(ls, l64)
    print(f'bfloat16 trunk: largest storage effect s = {s_max:.3e} (at {max(s, key=s.get)}), largest r_dev = {r_dev[worst]:.3e} at {worst} = '
          f'{r_dev[worst] / s_max:.2f} x s (bound: {FACTOR_BF16}); losses: device {max(r_loss.values()):.3e}, storage emulation {max(s_loss.values()):.3e}')
    assert set(grads) == set(g64) and all(g.dtype == torch.float32 for g in grads.values())
    late = {k: v for k, v in r_dev.items() if not v <= FACTOR_BF16 * s_max}
    assert s_max > 0 and not late, late
    losses2, grads2, _, _ = device_step(det, case, monkeypatch)
    assert all(torch.equal(losses[k], losses2[k]) for k in losses) and all(torch.equal(grads[k], grads2[k]) for k in grads)
