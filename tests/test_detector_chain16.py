"""Section 31's check for the fully 16-bit detector: one training step of Detector(train_dtype=bfloat16,
heads_train_dtype=bfloat16) on the GPU against tests/detector_chain16_ref.py, float64 torch.autograd on the CPU with a straight-through rounding
at every storage point of the trunk (section 30) and of the heads (section 32).

Yardstick, computed from the reference alone: s = the largest relative change that the roundings make in the float64 reference's parameter
gradients.  The device must stay within 2 x s for every parameter and map (section 31's own margin), and the set of parameters that hold a
gradient must be the reference's.  The decisions (matches, samples, RoIs, levels) are taken from the device run that is checked.  Run on section
31's cases small, four-levels (bfloat16 rows on all four RoI levels) and mixed (three frames, 1, 3 and 5 ground truths).  The test prints its
measured ratios before it asserts."""
import pytest
import torch

import detector_chain16_ref as cr16
import detector_chain_case as cc
import detector_chain_ref as cr
import dettrunk_case as tc
from test_detector_chain import BF16_CASES, FACTOR_BF16, detector, device_step, gradient_ratios, loss_ratios

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


@pytest.mark.parametrize('case', BF16_CASES)
def test_a_fully_bfloat16_training_step_stays_within_twice_the_storage_effect(case, monkeypatch):
    det = detector(case, train_from_stage=2, train_dtype=BF16, heads_train_dtype=BF16)
    assert det.trunk.train_dtype == BF16 and det.heads.train_dtype == BF16
    losses, grads, map_grads, inp = device_step(det, case, monkeypatch)               # the decisions of THIS run
    sd = tc.detector_weights()
    chain64 = cr.Chain(sd)
    l64, g64, m64 = chain64.step(inp)
    cc.check_reach(case, inp, chain64.kinks)
    # detector_chain16_ref's restated heads are detector_chain_ref's modules: with every rounding switched off they give its gradients
    plain = cr16.Chain16(sd, storage=None)
    monkeypatch.setattr(plain, '_hs', lambda x, fwd=True, bwd=True: x)
    lp, gp, mp = plain.step(inp)
    restated = max(gradient_ratios((gp, mp), (g64, m64)).values())
    print(f'the restated heads against the modules, no rounding: largest relative difference {restated:.3e}')
    assert restated <= 1e-12 and max(loss_ratios(lp, l64).values()) <= 1e-12
    ls, gs, ms = cr16.Chain16(sd).step(inp)
    s, r_dev = gradient_ratios((gs, ms), (g64, m64)), gradient_ratios((grads, map_grads), (g64, m64))
    s_max = max(v for k, v in s.items() if not k.startswith('map '))
    s_trunk = max(v for k, v in gradient_ratios(cr.Chain(sd, storage='bfloat16').step(inp)[1:], (g64, m64)).items() if not k.startswith('map '))
    worst = max(r_dev, key=r_dev.get)
    heads_only = {k: v for k, v in r_dev.items() if k.startswith('rpn.') or k.startswith('roi_heads.')}
    worst_head = max(heads_only, key=heads_only.get)
    r_loss, s_loss = loss_ratios(losses, l64), loss_ratios(ls, l64)
    print(f'fully bfloat16 on {case}: largest storage effect s = {s_max:.3e} (at {max(s, key=s.get)}; the trunk\'s roundings alone: {s_trunk:.3e}), largest r_dev = '
          f'{r_dev[worst]:.3e} at {worst} = {r_dev[worst] / s_max:.2f} x s (bound: {FACTOR_BF16}); over the heads\' parameters {heads_only[worst_head]:.3e} at '
          f'{worst_head}; losses: device {max(r_loss.values()):.3e}, storage emulation {max(s_loss.values()):.3e}')
    assert set(grads) == set(gs) == set(g64) == {k for k, _ in det.named_parameters()}
    assert all(g.dtype == torch.float32 for g in grads.values())
    late = {k: v for k, v in r_dev.items() if not v <= FACTOR_BF16 * s_max}
    assert s_max > 0 and not late, late
    losses2, grads2, map_grads2, _ = device_step(det, case, monkeypatch)              # a second run gives equal bits
    assert all(torch.equal(losses[k], losses2[k]) for k in losses) and all(torch.equal(grads[k], grads2[k]) for k in grads)
    assert all(torch.equal(a, b) for a, b in zip(map_grads, map_grads2))
