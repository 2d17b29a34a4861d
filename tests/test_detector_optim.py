"""The detector's optimiser on the GPU: cosy_sgd_step against its CPU twin, the pack table against the per-layer packs,
FlatSGD on a whole training step of the narrow detector, and train_detector_loop with a checkpointed resume."""
import types

import numpy as np
import pytest
import torch

import detector_chain_case as cc
import detopt_ref as ref
import dettrunk_case as tc
from cosypose_amd import Detector, FlatSGD, PackTable, _lib, train_detector_loop
from cosypose_amd.detector_heads import PackedOnDevice, TrainableLayer
from cosypose_amd.detector_trunk_backward import TrainableTrunkLayer
from cosypose_amd.training import LRSchedule, load_checkpoint

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
MIXES = {'float32': {}, 'bfloat16': dict(train_dtype=BF16, heads_train_dtype=BF16), 'bfloat16-trunk': dict(train_dtype=BF16)}
CASE = 'small'


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.detach().contiguous().view(-1).view(torch.uint8).cpu()


def detector(sd=None, **kw):
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in tc.detector_weights().items()} if sd is None else sd
    return Detector.from_state_dict(sd, tc.E2E_LABELS, input_resize=cc.CASES[CASE]['resize'], trainable=True, **kw)


def trainable_layers(det):
    return [l for l in det.trunk.layers() + det.heads.layers() if isinstance(l, PackedOnDevice)]


# ---- 1. the step kernel against the twin ----
def same_bits(got, want, what):
    """equal bits; IEEE 754 leaves the sign and payload of a NaN to the implementation (x86 generates a negative quiet NaN, gfx950 a positive
    one), so a NaN must sit where the twin has one and every other element must hold the twin's bits"""
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]), what
    return bool(np.array_equal(got.view(np.uint32), want.view(np.uint32)))


@pytest.mark.parametrize('case', list(ref.SCALARS))
def test_sgd_step_holds_the_twins_bits(case):
    lr, mu, wd = ref.SCALARS[case]
    L = _lib.lib()
    one_pass = int(L.cosy_sgd_step_pass_elements())
    assert one_pass > 0 and one_pass % 1024 == 0
    raw_equal = True
    for n in (1, 3, 4, 255, 257, one_pass + 5):
        for first in (True, False):
            w, g, m = ref.data(n, 100 + n % 97)
            want_w, want_m = ref.sgd_step(w, g, m, lr, mu, wd, first)
            dw, dg, dm = dev(w), dev(g), dev(m)
            _lib.check(L.cosy_sgd_step(dw.data_ptr(), dg.data_ptr(), dm.data_ptr(), n, lr, mu, wd, int(first), _lib.stream()))
            raw_equal &= same_bits(dw.cpu().numpy(), want_w, (case, n, first, 'w'))
            if mu == 0:
                assert torch.equal(bits(dm), bits(torch.from_numpy(m))), (case, n, first)          # untouched, the NaN's bits included
            else:
                raw_equal &= same_bits(dm.cpu().numpy(), want_m, (case, n, first, 'm'))
            assert torch.equal(bits(dg), bits(torch.from_numpy(g)))
    print(f'{case}: NaN signs and payloads equal the twin\'s too: {raw_equal}')


def test_sgd_step_without_momentum_takes_no_buffer():
    w, g, _ = ref.data(1030, 7)
    want, _ = ref.sgd_step(w, g, None, 0.02, 0.0, 1e-4, False)
    dw, dg = dev(w), dev(g)
    _lib.check(_lib.lib().cosy_sgd_step(dw.data_ptr(), dg.data_ptr(), None, 1030, 0.02, 0.0, 1e-4, 0, _lib.stream()))
    same_bits(dw.cpu().numpy(), want, 'w')


# ---- 2. the pack table against the per-layer packs ----
def packings(layer):
    return [bits(layer.w), bits(layer.bias), bits(layer.w_t)]


def fill(layers):
    for l in layers:
        for t in (l.w, l.bias, l.w_t):
            t.view(torch.uint8).fill_(0xFF)


def kind(l):
    if isinstance(l, TrainableTrunkLayer):
        return ('trunk', l.ksize, l.scale is not None)
    return (l.kind, l.ksize, len(l.pairs), tuple(int(w.shape[0]) for w, _ in l.pairs) if len(l.pairs) == 2 else None)


@pytest.mark.parametrize('mix', list(MIXES))
def test_pack_table_writes_the_per_layer_packs_bytes(mix):
    det = detector(**MIXES[mix])
    layers = trainable_layers(det)
    kinds = {kind(l) for l in layers}
    need = {('trunk', 1, True), ('trunk', 3, True), ('trunk', 1, False), ('trunk', 3, False), ('conv', 3, 1, None), ('linear', 1, 1, None), ('conv', 1, 2, (3, 12)),
            ('deconv', 1, 1, None)}
    assert need <= kinds and any(k[0] == 'linear' and k[2] == 2 for k in kinds), kinds
    assert {l.dtype for l in layers} == ({F32} if mix == 'float32' else {BF16} if mix == 'bfloat16' else {F32, BF16})
    fill(layers)
    for l in layers:
        l._pack()
    want = [packings(l) for l in layers]
    assert all((w[0] != 0xFF).any() for w in want)

    def check(order, tables):
        fill(layers)
        for t in tables:
            t.run()
        torch.cuda.synchronize()
        for i in order:
            for got, exp, name in zip(packings(layers[i]), want[i], ('w', 'bias', 'w_t')):
                assert torch.equal(got, exp), (mix, i, kind(layers[i]), name)
    everyone = list(range(len(layers)))
    check(everyone, [PackTable(layers)])
    check(everyone, [PackTable(layers[::-1])])
    check(everyone, [PackTable([l]) for l in layers])                 # tables of one layer


# ---- 3. FlatSGD on a whole step ----
def step_inputs():
    frames = [dev(f) for f in cc.frames(CASE)]
    targets = [{k: dev(v) for k, v in t.items()} for t in cc.targets(CASE)]
    keys = {name: dev(v) for name, v in cc.keys(CASE, cc.n_anchors(cc.padded_size(CASE))).items()}
    return frames, targets, keys


def forward(det):
    """the five maps and the heads' outputs on fixed inputs, under no_grad"""
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        maps = det.trunk(torch.randn(2, 3, 64, 64, generator=g).cuda())
        C = int(maps[0].shape[1])
        obj, dlt = det.heads.rpn_head(maps)
        out = list(maps) + list(obj) + list(dlt) + list(det.heads.box_head(torch.randn(5, C, 7, 7, generator=g).cuda()))
        out.append(det.heads.mask_head(torch.randn(3, C, 14, 14, generator=g).cuda()))
    return out


def count_packs(monkeypatch):
    calls = [0]
    for cls in (TrainableLayer, TrainableTrunkLayer):
        real = cls._pack

        def counted(self, real=real):
            calls[0] += 1
            return real(self)
        monkeypatch.setattr(cls, '_pack', counted)
    return calls


@pytest.mark.parametrize('mix', ['float32', 'bfloat16'])
def test_flat_sgd_step_keeps_every_packing_current(mix, monkeypatch):
    calls = count_packs(monkeypatch)
    frames, targets, keys = step_inputs()
    HYPER = dict(lr=0.01, momentum=0.9, weight_decay=1e-4)

    def run():
        det = detector(**MIXES[mix])
        sd0 = det.state_dict()
        named = det.named_parameters()
        opt = det.optimizer(**HYPER)
        assert [p for _, p in det.named_parameters()] == [p for _, p in named] and all(a is b for (_, a), (_, b) in zip(named, det.named_parameters()))
        sd1 = det.state_dict()
        assert sorted(sd0) == sorted(sd1) and all(torch.equal(bits(sd0[k]), bits(sd1[k])) for k in sd0)          # unchanged to the bit
        n_layers = len(opt.layers)
        assert n_layers == len(trainable_layers(det)) > 20
        det.zero_grad()                                                # .grad = None: the backward's fresh tensors are strays
        sum(det.losses(frames, targets, keys=keys).values()).backward()
        w, g = opt.flat.cpu().numpy().copy(), None
        count0, calls[0] = det.trunk.pack_count + det.heads.pack_count, 0
        norm = opt.step()
        g = opt.grad.cpu().numpy().copy()
        assert calls[0] == 0 and det.trunk.pack_count + det.heads.pack_count == count0 + n_layers
        assert float(norm) == pytest.approx(float(torch.linalg.vector_norm(opt.grad.double())), rel=1e-6) and float(norm) > 0
        want_w, want_m = ref.sgd_step(w, g, None, HYPER['lr'], HYPER['momentum'], HYPER['weight_decay'], first_step=True)
        same_bits(opt.flat.cpu().numpy(), want_w, 'flat'), same_bits(opt.momentum_buffer.cpu().numpy(), want_m, 'momentum')
        assert not np.array_equal(want_w, w)
        out = forward(det)                                              # the next forward: no per-layer pack
        assert calls[0] == 0 and det.trunk.pack_count + det.heads.pack_count == count0 + n_layers
        sum(det.losses(frames, targets, keys=keys).values())          # nor in the training forward
        assert calls[0] == 0
        sd2 = det.state_dict()
        other = detector(sd={k: v.cpu() for k, v in sd2.items()}, **MIXES[mix])
        for a, b in zip(out, forward(other)):
            assert torch.equal(bits(a), bits(b))
        assert calls[0] == n_layers                                     # the second detector packed layer by layer
        # a later load_state_dict moves the versions: the ordinary per-layer repack, and the first state's outputs
        calls[0] = 0
        det.load_state_dict(sd0)
        back = forward(det)
        assert calls[0] == n_layers and opt.owns()
        for a, b in zip(back, forward(detector(sd={k: v.cpu() for k, v in sd0.items()}, **MIXES[mix]))):
            assert torch.equal(bits(a), bits(b))
        return sd2, norm.clone(), out
    sd_a, norm_a, out_a = run()
    sd_b, norm_b, out_b = run()
    assert torch.equal(norm_a, norm_b) and all(torch.equal(bits(sd_a[k]), bits(sd_b[k])) for k in sd_a)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(out_a, out_b))


# ---- 4. the loop ----
def loop_cfg():
    """lr: the narrow detector's random weights give a total gradient norm of about 10^3, so a rate near the reference's 0.02 moves the
    parameters by several units a step and the losses overflow within four steps; 2e-5 moves them by about 0.02 a step and the losses fall"""
    return types.SimpleNamespace(lr=2e-5,momentum=0.9, weight_decay=1e-4, n_epochs_warmup=1, lr_epoch_decay=1, val_epoch_interval=1, rpn_box_reg_alpha=1,
                                 objectness_alpha=1, box_reg_alpha=1, classifier_alpha=1, mask_alpha=1)


def loop_batches():
    """two batches of the case's frames, on the CPU as a data loader hands them over: the second is the first in reverse order"""
    frames = [torch.from_numpy(f) for f in cc.frames(CASE)]
    targets = [{k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in t.items()} for t in cc.targets(CASE)]
    return [(frames, targets), (frames[::-1], targets[::-1])]


def test_train_detector_loop_and_its_resume(tmp_path):
    cfg, items, kw = loop_cfg(), loop_batches(), dict(train_dtype=BF16, heads_train_dtype=BF16)
    whole = detector(**kw)
    opt = whole.optimizer(lr=cfg.lr, momentum=cfg.momentum, weight_decay=cfg.weight_decay)
    seen, step = [], opt.step

    def recorded():
        opt._collect_stray_gradients()
        want = float(torch.linalg.vector_norm(opt.grad.double()))
        norm = step()
        seen.append((opt.param_groups[0]['lr'], float(norm), want))
        return norm
    opt.step = recorded
    log = {}
    history = train_detector_loop(whole, cfg, items, 2, optimizer=opt, val_batches=items[:1], on_epoch_end=lambda e, m: log.__setitem__(e, m), faithful_schedule=False,
                                  seed=4)
    for e, (rate, got, want) in enumerate(seen):
        print(f'step {e}: lr {rate:.6g}, grad_norm {got:.9g}, float64 norm of the flat gradient {want:.12g}')
    print({e: {k: round(v, 6) for k, v in m.items()} for e, m in log.items()})
    sched = LRSchedule(cfg.lr, 1, 2, 1, faithful=False)
    assert [s[0] for s in seen] == [sched.intended(e, b) for e in range(2) for b in range(2)]
    assert len(seen) == 4 and all(got == pytest.approx(want, rel=1e-6) and np.isfinite(want) and want > 0 for _, got, want in seen)
    for e in range(2):
        m = log[e]
        names = ('loss_rpn_box_reg', 'loss_objectness', 'loss_box_reg', 'loss_classifier', 'loss_mask', 'loss_total', 'grad_norm')
        assert all(f'train_{k}' in m and np.isfinite(m[f'train_{k}']) for k in names) and 'learning_rate' in m and 'val_loss_total' in m
        assert m['grad_norm'] == pytest.approx(np.mean([s[1] for s in seen[2 * e:2 * e + 2]]), rel=1e-6) and history[e] == m['train_loss_total']
        assert m['train_loss_total'] == pytest.approx(sum(m[f'train_{k}'] for k in names[:5]), rel=1e-5)
    # epoch 0, a checkpoint, a fresh detector, epoch 1: the bits of the uninterrupted run
    first = detector(**kw)
    train_detector_loop(first, cfg, items, 1, save_dir=tmp_path, faithful_schedule=False, save_optimizer=True, seed=4)
    resumed = detector(**kw)
    start = load_checkpoint(tmp_path, resumed)
    assert start == 1
    train_detector_loop(resumed, cfg, items, 2, save_dir=tmp_path, start_epoch=start, faithful_schedule=False, save_optimizer=True, seed=4)
    a, b = whole.state_dict(), resumed.state_dict()
    assert all(torch.equal(bits(a[k]), bits(b[k])) for k in a)
    assert not all(torch.equal(bits(a[k]), bits(v)) for k, v in first.state_dict().items())
