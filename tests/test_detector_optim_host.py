"""The detector's optimiser without a GPU: the CPU twin of cosy_sgd_step against torch.optim.SGD in float64, FlatSGD's
bookkeeping on CPU parameters, the gradient averaging across two gloo ranks, and the pack table's host validation."""
import ctypes
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import detopt_ref as ref
import detopt_gloo_worker


# ---- 1. the twin against torch.optim.SGD in float64 ----
@pytest.mark.parametrize('case', list(ref.SCALARS))
def test_twin_against_float64_torch_sgd(case):
    """4 steps; both sides start every step from the same float32 state (the float64 optimiser's momentum_buffer is set from the float32 one), so
    no error accumulates: the twin stays within the first-order bound of its own three (or fewer) roundings.  Pins the first-step buffer
    (m' = d), where the decay enters (into d, before the momentum), and that there is no dampening."""
    lr, mu, wd = ref.SCALARS[case]
    f32 = lambda v: float(np.float32(v))
    n = 4099
    w, _, _ = ref.data(n, 3, special=False)
    m = None
    worst_w = worst_m = 0.0
    for step in range(4):
        g = ref.data(n, 10 + step, special=False)[1]
        p64 = torch.nn.Parameter(torch.from_numpy(w.astype(np.float64)))
        opt = torch.optim.SGD([p64], lr=f32(lr), momentum=f32(mu), weight_decay=f32(wd))
        if step > 0 and mu != 0:
            opt.state[p64]['momentum_buffer'] = torch.from_numpy(m.astype(np.float64))
        p64.grad = torch.from_numpy(g.astype(np.float64))
        opt.step()
        w_new, m_new = ref.sgd_step(w, g, m, lr, mu, wd, first_step=step == 0)
        bw, bm = ref.bound(w, g, m, lr, mu, wd, first_step=step == 0)
        err_w = np.abs(w_new.astype(np.float64) - p64.detach().numpy())
        worst_w = max(worst_w, float((err_w / np.maximum(bw, 1e-300)).max()))
        assert (err_w <= bw).all(), (case, step, float((err_w / np.maximum(bw, 1e-300)).max()))
        if mu != 0:
            m64 = opt.state[p64]['momentum_buffer'].numpy()
            err_m = np.abs(m_new.astype(np.float64) - m64)
            assert (err_m <= bm).all(), (case, step)
            worst_m = max(worst_m, float((err_m / np.maximum(bm, 1e-300)).max()) if bm.max() > 0 else 0.0)
            if step == 0:
                d = g if wd == 0 else g + np.float32(wd) * w
                assert np.array_equal(m_new, d)                     # the first step's buffer is d itself, not (1 - dampening) d or mu 0 + d
        else:
            assert m_new is None and 'momentum_buffer' not in opt.state[p64]
        w, m = w_new, m_new
    print(f'{case}: largest error / bound: w {worst_w:.3f}, m {worst_m:.3f}')
    if case == 'lr=0':
        assert np.array_equal(w, ref.data(n, 3, special=False)[0])    # w - 0 m' is w, bit for bit


def test_twin_forms_no_product_it_does_not_need():
    """wd == 0 with an infinite weight and mu == 0 with a NaN buffer: the operation that would make a NaN is not performed"""
    w, g = np.array([np.inf, 1.0], np.float32), np.array([1.0, 2.0], np.float32)
    w1, m1 = ref.sgd_step(w, g, np.zeros(2, np.float32), 0.5, 0.9, 0.0, first_step=False)
    assert np.array_equal(m1, g) and w1[0] == np.inf and w1[1] == 0.0
    w2, m2 = ref.sgd_step(np.ones(2, np.float32), g, np.full(2, np.nan, np.float32), 0.5, 0.0, 0.0, first_step=False)
    assert m2 is None and np.array_equal(w2, np.array([0.5, 0.0], np.float32))


# ---- 2. bookkeeping on CPU parameters ----
SHAPES = [(3, 5), (7,), (2, 2, 3), (1,), (8, 4)]


class Holder:
    def __init__(self):
        g = torch.Generator().manual_seed(5)
        self.named = [(f'p{i}', torch.nn.Parameter(torch.randn(s, generator=g))) for i, s in enumerate(SHAPES)]

    def named_parameters(self):
        return list(self.named)


def test_flat_sgd_rehomes_the_parameters():
    from cosypose_amd import FlatSGD
    h = Holder()
    before = [(p, p.detach().clone()) for _, p in h.named]
    opt = FlatSGD(h, lr=0.1)
    off = 0
    for (p, value), o in zip(before, opt.offsets):
        assert o == off and o % 4 == 0                               # named_parameters() order, every start on 16 bytes
        assert p.data_ptr() == opt.flat.data_ptr() + 4 * o and p.data_ptr() % 16 == 0
        assert p.grad.data_ptr() == opt.grad.data_ptr() + 4 * o and p.grad.shape == p.shape
        assert torch.equal(p.detach(), value) and isinstance(p, torch.nn.Parameter) and p.requires_grad
        off += -(-p.numel() // 4) * 4
    assert [p for _, p in h.named] == [p for p, _ in before] and all(a is b for (_, a), (b, _) in zip(h.named, before))      # identity kept
    assert opt.flat.numel() == off == opt.grad.numel()
    used = torch.zeros(off, dtype=torch.bool)
    for (p, _), o in zip(before, opt.offsets):
        used[o:o + p.numel()] = True
    assert (~used).any() and (opt.flat[~used] == 0).all() and (opt.grad == 0).all()
    assert opt.param_groups[0]['lr'] == 0.1 and opt.owns()
    # autograd accumulates into the views in place
    loss = sum((p * p).sum() for _, p in h.named)
    loss.backward()
    for (p, value), o in zip(before, opt.offsets):
        assert p.grad.data_ptr() == opt.grad.data_ptr() + 4 * o and torch.equal(opt.grad[o:o + p.numel()].view(p.shape), 2 * value)
    assert (opt.grad[~used] == 0).all()


def test_flat_sgd_collects_stray_gradients_and_zero_grad_reattaches():
    from cosypose_amd import FlatSGD
    h = Holder()
    params = [p for _, p in h.named]
    opt = FlatSGD(params, lr=0.1, momentum=0.0, weight_decay=0.0)
    with torch.no_grad():
        for p in params:
            p.grad.fill_(1.0)
    params[0].grad = None                                            # Detector.zero_grad()
    foreign = torch.full(SHAPES[2], 7.0)
    params[2].grad = None
    params[2].grad = foreign                                         # a backward after it allocated a fresh tensor
    opt._collect_stray_gradients()
    for i, (p, o) in enumerate(zip(params, opt.offsets)):
        assert p.grad.data_ptr() == opt.grad.data_ptr() + 4 * o
        assert torch.equal(p.grad, torch.full(SHAPES[i], {0: 0.0, 2: 7.0}.get(i, 1.0)))
    params[1].grad = None
    params[4].grad = None
    params[4].grad = torch.ones(SHAPES[4])
    opt.zero_grad()
    assert (opt.grad == 0).all()
    for p, o in zip(params, opt.offsets):
        assert p.grad.data_ptr() == opt.grad.data_ptr() + 4 * o and (p.grad == 0).all()


def test_flat_sgd_step_on_the_cpu_raises():
    from cosypose_amd import FlatSGD, _lib
    opt = FlatSGD(Holder(), lr=0.1)
    with pytest.raises(_lib.CosyHipError, match='no CPU fallback'):
        opt.step()


def test_flat_sgd_refuses_what_it_cannot_hold():
    from cosypose_amd import FlatSGD
    with pytest.raises(ValueError, match='float32'):
        FlatSGD([torch.nn.Parameter(torch.zeros(3, dtype=torch.float64))], lr=0.1)
    p = torch.nn.Parameter(torch.zeros(3))
    with pytest.raises(ValueError, match='twice'):
        FlatSGD([p, p], lr=0.1)
    with pytest.raises(ValueError, match='>= 0'):
        FlatSGD([p], lr=-1.0)
    with pytest.raises(ValueError, match='PackedOnDevice'):
        FlatSGD([p], lr=0.1, layers=[object()])


def test_lr_schedule_sets_the_rate_through_param_groups():
    from cosypose_amd import FlatSGD
    from cosypose_amd.training import LRSchedule
    opt = FlatSGD(Holder(), lr=0.5)
    s = LRSchedule(0.02, 1, 4, 2)
    assert s.apply(opt, 0, 0) == opt.param_groups[0]['lr'] == 0.02 / 4


# ---- 3. two gloo ranks ----
def test_allreduce_gradients_of_a_flat_sgd_two_gloo_ranks():
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=detopt_gloo_worker.worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=180) for _ in range(2))
    for p in procs:
        p.join(60)
    assert res == [(0, True), (1, True)]


def test_allreduce_gradients_keeps_its_other_arguments():
    from cosypose_amd.train_engine import allreduce_gradients
    g = torch.arange(5.0)
    assert allreduce_gradients(g) is g and torch.equal(g, torch.arange(5.0))      # no process group: the buffer as it is
    with pytest.raises(TypeError, match='FlatSGD'):
        allreduce_gradients([g])


# ---- 5. the pack table's host validation: the built library, no device ----
def _row(**kw):
    """a valid row over made-up addresses (nothing is dereferenced: the refusal comes before anything touches the device)"""
    r = dict(w0=0x1000, b0=0x2000, w1=0, b1=0, scale=0, fwd=0x3000, fwd_bias=0x4000, bwd=0x5000, ksize=3, c_in=16, n0=8, n1=0, dtype=0)
    r.update(kw)
    return [r[k] for k in ('w0', 'b0', 'w1', 'b1', 'scale', 'fwd', 'fwd_bias', 'bwd', 'ksize', 'c_in', 'n0', 'n1', 'dtype')]


BAD_ROWS = {
    'null pointer': (dict(b0=0), 'null b0'),
    'null packing': (dict(bwd=0), 'null bwd'),
    'c_in not a multiple of 8': (dict(c_in=12), 'c_in=12'),
    'deconvolution with a sibling': (dict(ksize=2, n1=8, w1=0x6000, b1=0x7000), 'a deconvolution has no sibling'),
    'unaligned packing': (dict(fwd=0x3008), '16-byte aligned'),
    'sibling without its tensors': (dict(n1=4), 'null w1 or b1'),
    'float16 rows': (dict(dtype=2), 'dtype=2'),
    'scale with a sibling': (dict(scale=0x8000, n1=8, w1=0x6000, b1=0x7000), 'a layer with a scale'),
}


@pytest.mark.parametrize('what', list(BAD_ROWS))
def test_pack_table_build_refuses_a_bad_row(what):
    from cosypose_amd import _lib
    from cosypose_amd.build import build
    build()
    L = _lib.lib()
    change, message = BAD_ROWS[what]
    rows = _row() + _row(**change)                                   # the second layer is the bad one: the message says which
    n = ctypes.c_longlong(-1)
    rc = L.cosy_pack_table_build((ctypes.c_longlong * len(rows))(*rows), 2, 0x10000, L.cosy_pack_table_bytes(2), ctypes.byref(n), None)
    err = L.cosy_last_error().decode()
    assert rc != 0 and err.startswith('cosy_pack_table_build: layer 1:') and message in err, err
    assert n.value == -1


def test_pack_table_build_checks_its_own_arguments():
    from cosypose_amd import _lib
    from cosypose_amd.build import build
    build()
    L = _lib.lib()
    rows = (ctypes.c_longlong * 13)(*_row())
    n = ctypes.c_longlong(0)
    assert L.cosy_pack_table_bytes(0) == 0 and L.cosy_pack_table_bytes(4097) == 0 and L.cosy_pack_table_bytes(2) > L.cosy_pack_table_bytes(1) > 0
    for args, message in (((rows, 0, 0x10000, 1 << 20, ctypes.byref(n), None), 'n_layers=0'), ((None, 1, 0x10000, 1 << 20, ctypes.byref(n), None), 'null rows'),
                          ((rows, 1, None, 1 << 20, ctypes.byref(n), None), 'null table'), ((rows, 1, 0x10008, 1 << 20, ctypes.byref(n), None), '16-byte'),
                          ((rows, 1, 0x10000, 8, ctypes.byref(n), None), 'table_bytes=8')):
        assert L.cosy_pack_table_build(*args) != 0
        err = L.cosy_last_error().decode()
        assert err.startswith('cosy_pack_table_build:') and message in err, err
    assert L.cosy_pack_table_run(None, 1, 1, None) != 0 and L.cosy_last_error().decode().startswith('cosy_pack_table_run: null table')
    assert L.cosy_pack_table_run(0x10000, 1, 0, None) != 0 and 'n_workgroups=0' in L.cosy_last_error().decode()
    assert L.cosy_sgd_step(None, None, None, -1, 0.1, 0.9, 0.0, 1, None) != 0 and L.cosy_last_error().decode().startswith('cosy_sgd_step: n=-1')
    assert L.cosy_sgd_step(0x1000, 0x2000, None, 8, 0.1, 0.9, 0.0, 1, None) != 0 and 'null momentum_buf' in L.cosy_last_error().decode()
    assert L.cosy_sgd_step(0x1004, 0x2000, None, 8, 0.1, 0.0, 0.0, 1, None) != 0 and '16-byte aligned' in L.cosy_last_error().decode()
    assert L.cosy_sgd_step(None, None, None, 0, 0.1, 0.9, 0.0, 1, None) == 0           # nothing to do
