"""The loop around the detector's training step without a GPU: h_maskrcnn's weighting and train_detector_loop's order of
operations on a stub detector whose losses are a function of one small CPU parameter, against the reference's loop written out here with torch's
own schedulers."""
import types
import warnings
from collections import defaultdict

import pytest
import torch

from cosypose_amd import h_maskrcnn, train_detector_loop
from cosypose_amd.detector_training import LOSSES, optimizer_path
from cosypose_amd.training import LazyMeters, _Mean, checkpoint_path, load_checkpoint

ALPHA = dict(rpn_box_reg_alpha=1.5, objectness_alpha=0.25, box_reg_alpha=3.0, classifier_alpha=0.75, mask_alpha=2.0)


def cfg(**kw):
    base = dict(lr=0.05, momentum=0.9, weight_decay=1e-3, n_epochs_warmup=1, lr_epoch_decay=1, val_epoch_interval=2, **ALPHA)
    base.update(kw)
    return types.SimpleNamespace(**base)


class FixedLosses:
    """a detector that returns five fixed CPU losses and records what it was given"""

    def __init__(self):
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.values = dict(zip(LOSSES, (0.5, 1.25, 2.0, 0.125, 3.0)))

    def parameters(self):
        return [self.p]

    def losses(self, frames, targets, generator=None):
        self.seen = (frames, targets, generator)
        return {k: torch.tensor(v) + 0 * self.p.sum() for k, v in self.values.items()}


class Quadratic:
    """losses that depend on the frames and on a small parameter: loss_i = c_i sum((p - x_i)^2), x_i the mean of frame i mod len(frames)"""

    def __init__(self):
        self.p = torch.nn.Parameter(torch.tensor([0.3, -1.2, 2.5, 0.01, -0.7]))

    def parameters(self):
        return [self.p]

    def named_parameters(self):
        return [('p', self.p)]

    def state_dict(self):
        return {'p': self.p.detach().clone()}

    def load_state_dict(self, sd, strict=True):
        with torch.no_grad():
            self.p.copy_(sd['p'])

    def losses(self, frames, targets, generator=None):
        out = {}
        for i, k in enumerate(LOSSES):
            x = frames[i % len(frames)].float().mean() / 255
            out[k] = (0.5 + 0.25 * i) * ((self.p - x) ** 2).sum()
        return out


def batches(n=2):
    g = torch.Generator().manual_seed(9)
    out = []
    for _ in range(n):
        frames = [torch.randint(0, 256, (6, 8, 3), dtype=torch.uint8, generator=g) for _ in range(2)]
        targets = [dict(boxes=torch.tensor([[1.0, 1.0, 5.0, 4.0]]), labels=torch.tensor([1]), masks=torch.ones(1, 6, 8, dtype=torch.uint8)) for _ in range(2)]
        out.append((frames, targets))
    return out


def weighted(loss_dict, c):
    return (c.rpn_box_reg_alpha * loss_dict['loss_rpn_box_reg'] + c.objectness_alpha * loss_dict['loss_objectness'] + c.box_reg_alpha * loss_dict['loss_box_reg'] +
            c.classifier_alpha * loss_dict['loss_classifier'] + c.mask_alpha * loss_dict['loss_mask'])


@pytest.mark.parametrize('meters', [lambda: defaultdict(_Mean), lambda: LazyMeters(_Mean)])
def test_h_maskrcnn_weights_the_five_losses_and_fills_their_meters(meters):
    det, c, m = FixedLosses(), cfg(), meters()
    gen = torch.Generator()
    data = batches(1)[0]
    loss = h_maskrcnn(data, det, m, c, generator=gen)
    assert torch.equal(loss.detach(), weighted({k: torch.tensor(v) for k, v in det.values.items()}, c)) and loss.requires_grad
    assert {k: m[k].mean for k in LOSSES} == det.values and all(m[k].n == 1 for k in LOSSES) and 'loss_total' not in m
    frames, targets, seen_gen = det.seen
    assert seen_gen is gen and all(f.dtype == torch.uint8 and f.shape == (6, 8, 3) for f in frames) and all(a is b for a, b in zip(frames, data[0]))
    assert [sorted(t) for t in targets] == [['boxes', 'labels', 'masks']] * 2


def reference_loop(det, c, items, start_epoch, n_epochs):
    """cosypose/training/train_detector.py:206-275 on the stub: SGD, the LambdaLR with its resume fast-forward, the StepLR, and the step"""
    bpe = len(items)
    opt = torch.optim.SGD(det.parameters(), lr=c.lr, weight_decay=c.weight_decay, momentum=c.momentum)
    nbw = c.n_epochs_warmup * bpe
    lambd = (lambda e: 1) if c.n_epochs_warmup == 0 else (lambda b: (b + 1) / nbw)
    warm = torch.optim.lr_scheduler.LambdaLR(opt, lambd)
    warm.last_epoch = start_epoch * bpe
    sch = torch.optim.lr_scheduler.StepLR(opt, step_size=c.lr_epoch_decay, gamma=0.1)
    sch.last_epoch = start_epoch - 1
    sch.step()
    rates, norms = [], []
    for epoch in range(start_epoch, n_epochs):
        for frames, targets in items:
            opt.zero_grad()
            loss = weighted(det.losses(frames, targets), c)
            loss.backward()
            norms.append(float(torch.nn.utils.clip_grad_norm_(det.parameters(), max_norm=float('inf'), norm_type=2)))
            rates.append(opt.param_groups[0]['lr'])
            opt.step()
            if epoch < c.n_epochs_warmup:
                warm.step()
        if epoch >= c.n_epochs_warmup:
            sch.step()
    return rates, norms, opt.param_groups[0]['lr']


def recording_sgd(det, c):
    opt = torch.optim.SGD(det.parameters(), lr=c.lr, weight_decay=c.weight_decay, momentum=c.momentum)
    rates, step = [], opt.step

    def recorded(*a, **kw):
        rates.append(opt.param_groups[0]['lr'])
        return step(*a, **kw)
    opt.step = recorded
    return opt, rates


@pytest.mark.parametrize('start_epoch, n_warm', [(0, 1), (0, 0), (1, 1), (2, 1)])
def test_loop_against_the_reference_loop_with_torch_schedulers(start_epoch, n_warm):
    """3 epochs of 2 batches, fresh (with and without warm-up) and resumed with the faithful schedule: the parameters are bit-equal to the
    reference's loop, the learning rates that reached the step and the logged values too"""
    c, items = cfg(n_epochs_warmup=n_warm), batches(2)
    n_epochs = start_epoch + 3
    want = Quadratic()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        want_rates, want_norms, want_last = reference_loop(want, c, items, start_epoch, n_epochs)
    got = Quadratic()
    opt, rates = recording_sgd(got, c)
    log = {}
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        history = train_detector_loop(got, c, items, n_epochs, start_epoch=start_epoch, optimizer=opt, on_epoch_end=lambda e, m: log.__setitem__(e, m),
                                      val_batches=items[:1], faithful_schedule=True)
    assert any('faithful_schedule' in str(w.message) for w in caught) == (start_epoch > 0)
    assert torch.equal(got.p.detach(), want.p.detach()), (got.p, want.p)
    assert rates == want_rates and len(rates) == 6
    assert sorted(history) == sorted(log) == list(range(start_epoch, n_epochs))
    for i, e in enumerate(range(start_epoch, n_epochs)):
        m = log[e]
        assert {'grad_norm', 'learning_rate', 'train_loss_total', 'train_grad_norm'} | {f'train_{k}' for k in LOSSES} <= set(m)
        assert m['grad_norm'] == pytest.approx(sum(want_norms[2 * i:2 * i + 2]) / 2, rel=1e-6) and history[e] == m['train_loss_total']
        assert ('val_loss_total' in m) == (e % c.val_epoch_interval == 0) and ('val_loss_mask' in m) == (e % c.val_epoch_interval == 0)
    assert log[n_epochs - 1]['learning_rate'] == want_last


def test_validation_leaves_the_training_untouched():
    c, items = cfg(), batches(2)
    a, b = Quadratic(), Quadratic()
    train_detector_loop(a, c, items, 2, optimizer=recording_sgd(a, c)[0])
    train_detector_loop(b, c, items, 2, optimizer=recording_sgd(b, c)[0], val_batches=items)
    assert torch.equal(a.p.detach(), b.p.detach()) and b.p.grad is not None


def test_checkpoint_and_optimizer_round_trip(tmp_path):
    """an interrupted run with save_optimizer=True and the intended schedule continues bit for bit; without the optimiser file the momentum restarts"""
    c, items = cfg(), batches(2)
    whole = Quadratic()
    train_detector_loop(whole, c, items, 3, optimizer=recording_sgd(whole, c)[0], faithful_schedule=False)
    first = Quadratic()
    train_detector_loop(first, c, items, 2, save_dir=tmp_path, optimizer=recording_sgd(first, c)[0], faithful_schedule=False, save_optimizer=True)
    assert checkpoint_path(tmp_path).exists() and optimizer_path(tmp_path).exists()
    save = torch.load(checkpoint_path(tmp_path))
    assert sorted(save) == ['epoch', 'state_dict'] and save['epoch'] == 1 and torch.equal(save['state_dict']['p'], first.p.detach())
    resumed = Quadratic()
    start = load_checkpoint(tmp_path, resumed)
    assert start == 2 and torch.equal(resumed.p.detach(), first.p.detach())
    train_detector_loop(resumed, c, items, 3, save_dir=tmp_path, start_epoch=start, optimizer=recording_sgd(resumed, c)[0], faithful_schedule=False, save_optimizer=True)
    assert torch.equal(resumed.p.detach(), whole.p.detach())
    assert torch.load(checkpoint_path(tmp_path))['epoch'] == 2
    cold = Quadratic()
    cold.load_state_dict(first.state_dict())
    train_detector_loop(cold, c, items, 3, start_epoch=2, optimizer=recording_sgd(cold, c)[0], faithful_schedule=False)      # the reference: empty momentum
    assert not torch.equal(cold.p.detach(), whole.p.detach())


def test_flat_sgd_state_round_trip_on_the_cpu():
    from cosypose_amd import FlatSGD
    a = FlatSGD([torch.nn.Parameter(torch.ones(5))], lr=0.1)
    a.momentum_buffer.copy_(torch.arange(8.0))
    a.step_count = 3
    a.param_groups[0]['lr'] = 0.25
    state = a.state_dict()
    b = FlatSGD([torch.nn.Parameter(torch.ones(5))], lr=0.1)
    b.load_state_dict(state)
    assert torch.equal(b.momentum_buffer, torch.arange(8.0)) and b.step_count == 3 and b.param_groups[0]['lr'] == 0.25
    assert FlatSGD([torch.nn.Parameter(torch.ones(5))], lr=0.1).state_dict()['momentum_buffer'] is None          # before the first step
    with pytest.raises(ValueError, match='does not fit'):
        FlatSGD([torch.nn.Parameter(torch.ones(50))], lr=0.1).load_state_dict(state)
