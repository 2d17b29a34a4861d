"""Kernel-level parity of the training step (csrc/kernels_train.hip) against float64 torch on the CPU.

The end-to-end training tests (test_gpu_parity.py: test_training_step_vs_reference, ..._with_drop_connect, ..._batch64_vs_oracle)
run one crop size and judge 340 gradient tensors after 26 blocks of error build-up.  Here the training entries of the C ABI are
held on their own, except those that run on the matrix instruction, which live in test_train_matrix_kernels.py (cosy_train_gemm,
cosy_train_gemm_packed with cosy_train_pack_plan / _pack_all, cosy_wgrad, cosy_se_train_forward / _backward, cosy_fc_small_forward /
_backward, cosy_rows_mean_bn / cosy_rows_dot_bn).  The reference restates the OPERATION in float64 with stock torch on the CPU (F.conv2d on the statically padded
input, F.batch_norm + x * sigmoid(x) with autograd, clip_grad_norm_ + Adam, TorchRef.disentangled_loss with autograd), from the
same fp32 inputs the kernel gets, at the network's 14 depthwise shape classes (EfficientNet-B3 at 240x320) and 256x256's 8x8
maps, plus ragged shapes where the kernels' tails live (Ho % 4 != 0 for the 4-row depthwise threads, Wo % 4 != 0 for the 4-pixel
weight-gradient runs, odd sides and the minimal 2- and 3-pixel inputs at stride 2, C = 4, C = 68 = one quad in the second
64-channel group, C = 2304, B = 1 / 3 / 16).  Every reduction claims a fixed order without atomics: each is re-run once and
compared with torch.equal.

Errors are max |kernel - float64| / max |float64| over a tensor unless stated; every case prints its measured value (-s).
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cosypose_amd import arch

pytestmark = pytest.mark.gpu

COSY_OK, COSY_EINVAL = 0, -1
BN_EPS, BN_MOM = 1e-3, 0.01
f32 = lambda v: float(np.float32(v))          # a hyperparameter as the C ABI receives it


def _te():
    from cosypose_amd import train_engine
    return train_engine


def _abi():
    from cosypose_amd._lib import lib, ptr, stream
    return lib(), ptr, stream


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def dev(t):
    return t.contiguous().to('cuda')


def rel(got, want):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    return float((got - want).abs().max() / max(float(want.abs().max()), 1e-30))


def report(tag, err, bound):
    print(f'  {tag}: {err:.3g} (bound {bound:g})')
    assert err < bound, (tag, err, bound)


# ---------------------------------------------------------------------------------------------------------------------------
# BatchNorm in train mode
# ---------------------------------------------------------------------------------------------------------------------------
BN_STATS_TOL = 1.5e-7        # mean / rstd / running stats: one fp32 rounding of double sums (measured 5.7e-8)
BN_STATS_CASES = [(2, 1536, 0), (63, 68, 0), (64, 4, 0), (65, 816, 0), (129, 40, 0), (4480, 68, 0), (4480, 816, 100),
                  (4480, 1536, 0), (16 * 120 * 160, 40, 0)]


@pytest.mark.parametrize('M,C,mu', BN_STATS_CASES)
def test_bn_stats_vs_fp64(M, C, mu):
    """cosy_bn_train_stats: batch mean and 1/sqrt(biased variance + 1e-3) per channel, running_mean / running_var after one
    update with momentum 0.01 and the UNBIASED variance from non-zero values (F.batch_norm's own update); M = 2 .. 16x120x160
    rows, C = 4 .. 1536, one case with per-channel mean = 100 sigma (a one-pass variance would cancel there).  Null running
    pointers: the call succeeds and gives the same mean and rstd, bit for bit (which is also the re-run check).
    Measured worst: mean 5.3e-8, rstd 5.1e-8, running_mean 5.7e-8, running_var 4.0e-8 (bound 1.5e-7)."""
    te = _te()
    lib, ptr, stream = _abi()
    g = _gen(M * 7 + C)
    sig = torch.rand(C, generator=g) * 1.5 + 0.5
    shift = mu * sig if mu else torch.randn(C, generator=g) * 0.5
    x = torch.randn(M, C, generator=g) * sig + shift
    rm0, rv0 = torch.randn(C, generator=g) * 0.3, torch.rand(C, generator=g) + 0.5
    xd, rm, rv = dev(x), dev(rm0), dev(rv0)
    mean, rstd = te.bn_stats(xd, M, C, rm, rv)
    x64 = x.double()
    var, m64 = torch.var_mean(x64, 0, unbiased=False)
    rm64, rv64 = rm0.double(), rv0.double()
    F.batch_norm(x64.t().unsqueeze(0), rm64, rv64, None, None, True, BN_MOM, BN_EPS)      # updates rm64 / rv64 in place
    report(f'M={M} C={C} mean', rel(mean, m64), BN_STATS_TOL)
    report(f'M={M} C={C} rstd', rel(rstd, 1.0 / torch.sqrt(var + BN_EPS)), BN_STATS_TOL)
    report(f'M={M} C={C} running_mean', rel(rm, rm64), BN_STATS_TOL)
    report(f'M={M} C={C} running_var', rel(rv, rv64), BN_STATS_TOL)
    mean2, rstd2 = torch.full_like(mean, 7.0), torch.full_like(rstd, 7.0)
    rc = lib.cosy_bn_train_stats(ptr(xd), M, C, BN_EPS, BN_MOM, ptr(mean2), ptr(rstd2), None, None, ptr(te._workspace(xd.device)), stream())
    assert rc == COSY_OK
    assert torch.equal(mean2, mean) and torch.equal(rstd2, rstd)


BN_TOL = 5e-7                # apply: elementwise (measured 1.8e-7)
BN_DX_TOL = 1e-6             # dx: elementwise, from this call's per-channel sums (measured 3.4e-7)
BN_SUM_TOL = 5e-7            # dgamma / dbeta: per-channel sums over up to 3 x 10^5 rows (measured 2.0e-7)
# gated form: the incoming gradient dout * gate + add / HW is formed per element in fp32 and its rounding is biased over the HW rows
# of one sample -- an fp32 CPU evaluation of that product alone is 1.1e-6 off in dbeta at HW = 19200 (measured 2.0e-6)
BN_GATED_SUM_TOL = 5e-6
BN_SHAPES = [(3, 1, 1536), (16, 1, 68), (1, 70, 816), (3, 70, 68), (16, 70, 40), (1, 19200, 40), (3, 19200, 4), (16, 19200, 24)]


def _bn_case(B, HW, C):
    g = _gen(B * 100003 + HW * 7 + C)
    M = B * HW
    x = torch.randn(M, C, generator=g) * (torch.rand(C, generator=g) + 0.5) + torch.randn(C, generator=g) * 0.5
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g) * 0.5
    keep = 0.7
    rowscale = torch.tensor([0.0 if b % 3 == 1 else 1.0 / keep for b in range(B)], dtype=torch.float32)   # drop_connect: zeros and 1/keep
    res, dout = torch.randn(M, C, generator=g), torch.randn(M, C, generator=g)
    cgate, cadd = torch.sigmoid(torch.randn(B, C, generator=g)), torch.randn(B, C, generator=g)
    return x, gamma, beta, rowscale, res, dout, cgate, cadd


def _bn_ref(x, gamma, beta, B, HW, act):
    """act(F.batch_norm(x)) in train mode, x (B*HW, C) as the (B, C, HW) batch it is"""
    C = x.shape[1]
    y = F.batch_norm(x.view(B, HW, C).permute(0, 2, 1), None, None, gamma, beta, True, BN_MOM, BN_EPS).permute(0, 2, 1).reshape(B * HW, C)
    return y * torch.sigmoid(y) if act else y


@pytest.mark.parametrize('B,HW,C', BN_SHAPES)
def test_bn_apply_vs_fp64(B, HW, C):
    """cosy_bn_train_apply (act 0 / 1 x rowscale none / per sample with zeros and 1/keep x res none / tensor) and
    cosy_bn_train_apply_gated on the kernel's own statistics, against drop_connect(swish(F.batch_norm(x))) + res and
    swish(bn(x)) * gate[sample] in float64.  Measured worst: 1.8e-7 (bound 5e-7)."""
    te = _te()
    x, gamma, beta, rowscale, res, _, cgate, _ = _bn_case(B, HW, C)
    M = B * HW
    xd, gd, bd, rsd, resd, cgd = dev(x), dev(gamma), dev(beta), dev(rowscale), dev(res), dev(cgate)
    mean, rstd = te.bn_stats(xd, M, C)
    rs_rows = rowscale.double().repeat_interleave(HW)[:, None]
    for act in (0, 1):
        y = _bn_ref(x.double(), gamma.double(), beta.double(), B, HW, act)
        for scaled in (False, True):
            for with_res in (False, True):
                want = (y * rs_rows if scaled else y) + (res.double() if with_res else 0.0)
                got = te.bn_apply(xd, mean, rstd, gd, bd, M, C, act, rsd if scaled else None, HW, resd if with_res else None)
                report(f'B={B} HW={HW} C={C} act={act} rowscale={int(scaled)} res={int(with_res)}', rel(got, want), BN_TOL)
        got = te.bn_apply_gated(xd, mean, rstd, gd, bd, M, C, act, cgd, HW)
        report(f'B={B} HW={HW} C={C} act={act} gated', rel(got, y * cgate.double().repeat_interleave(HW, 0)), BN_TOL)


@pytest.mark.parametrize('B,HW,C', BN_SHAPES)
def test_bn_backward_vs_fp64(B, HW, C):
    """cosy_bn_train_backward_gated (act 0 / 1; rowscale; the gated form dout * cgate[sample] + cadd[sample] / HW) against float64
    autograd of the forward above: dx, dgamma, dbeta.  The raw cosy_bn_train_backward with accumulate = 1 on non-zero dgamma /
    dbeta: the old values plus this call's sums (bit for bit: one fp32 add), `sums` = this call's sums only, dx bit-identical
    (which is also the re-run check).  Measured worst: dx 3.4e-7 (bound 1e-6); dgamma / dbeta 2.0e-7 (bound 5e-7), gated form
    2.0e-6 (bound 5e-6, see BN_GATED_SUM_TOL)."""
    te = _te()
    lib, ptr, stream = _abi()
    x, gamma, beta, rowscale, _, dout, cgate, cadd = _bn_case(B, HW, C)
    M = B * HW
    xd, gd, bd, rsd, dd, cgd, cad = dev(x), dev(gamma), dev(beta), dev(rowscale), dev(dout), dev(cgate), dev(cadd)
    mean, rstd = te.bn_stats(xd, M, C)
    cadd_scale = f32(1.0 / HW)
    g = _gen(B + HW + C)
    for act in (0, 1):
        for form in ('plain', 'rowscale', 'gated'):
            x64, g64, b64 = (t.double().requires_grad_(True) for t in (x, gamma, beta))
            y = _bn_ref(x64, g64, b64, B, HW, act)
            if form == 'rowscale':
                y = y * rowscale.double().repeat_interleave(HW)[:, None]
            up = dout.double()
            if form == 'gated':
                up = up * cgate.double().repeat_interleave(HW, 0) + cadd.double().repeat_interleave(HW, 0) * cadd_scale
            y.backward(up)
            kw = dict(HW=HW, cgate=cgd, cadd=cad, cadd_scale=cadd_scale) if form == 'gated' else \
                dict(rowscale=rsd if form == 'rowscale' else None, HW=HW)
            dx, dg, db = te.bn_backward(dd, xd, mean, rstd, gd, bd, M, C, act, **kw)
            tag = f'B={B} HW={HW} C={C} act={act} {form}'
            sum_tol = BN_GATED_SUM_TOL if form == 'gated' else BN_SUM_TOL
            report(tag + ' dx', rel(dx, x64.grad), BN_DX_TOL)
            report(tag + ' dgamma', rel(dg, g64.grad), sum_tol)
            report(tag + ' dbeta', rel(db, b64.grad), sum_tol)
            if form == 'gated':
                continue
            # the raw ABI, accumulating into existing parameter gradients
            dg0, db0 = torch.randn(C, generator=g), torch.randn(C, generator=g)
            dga, dba, dx2, sums = dev(dg0), dev(db0), torch.empty_like(xd), torch.empty(2 * C, device='cuda')
            rc = lib.cosy_bn_train_backward(ptr(dd), ptr(xd), ptr(mean), ptr(rstd), ptr(gd), ptr(bd), M, C, act,
                                            ptr(rsd if form == 'rowscale' else None), HW, ptr(dga), ptr(dba), 1, ptr(dx2), ptr(sums),
                                            ptr(te._workspace(xd.device)), stream())
            assert rc == COSY_OK
            assert torch.equal(sums[:C], db) and torch.equal(sums[C:], dg)
            assert torch.equal(dga, dev(dg0) + dg) and torch.equal(dba, dev(db0) + db)
            assert torch.equal(dx2, dx)
            report(tag + ' accumulated dgamma', rel(dga, dg0.double() + g64.grad), BN_SUM_TOL)


# ---------------------------------------------------------------------------------------------------------------------------
# depthwise convolution
# ---------------------------------------------------------------------------------------------------------------------------
def _network_dw_shapes():
    """the (H, W, C, k, s) of every depthwise layer of EfficientNet-B3 at 240x320 (14 classes), from arch"""
    out, (h, w) = [], (arch.conv_out(240, 3, 2), arch.conv_out(320, 3, 2))
    for k, s, e, cin, cout in arch.B3_BLOCKS:
        if (h, w, cin * e, k, s) not in out:
            out.append((h, w, cin * e, k, s))
        h, w = arch.conv_out(h, k, s), arch.conv_out(w, k, s)
    return out


NETWORK_DW = _network_dw_shapes()
assert len(NETWORK_DW) == 14
DW_CASES = [(2,) + t for t in NETWORK_DW] + [
    (2, 8, 8, 1392, 5, 1), (2, 8, 8, 2304, 3, 1),                    # 256x256: the 8x8 final maps
    (1, 9, 7, 68, 3, 1), (3, 13, 9, 4, 5, 1), (1, 9, 7, 2304, 5, 1),  # Ho, Wo not multiples of 4; C = 4, 68, 2304
    (3, 7, 10, 68, 3, 2), (1, 19, 15, 68, 3, 2), (3, 17, 13, 4, 5, 2), (3, 5, 6, 2304, 3, 2),   # odd / ragged sides at stride 2
    (1, 2, 3, 4, 3, 2), (3, 3, 2, 68, 5, 2), (1, 2, 9, 8, 5, 2), (3, 11, 3, 4, 3, 2),           # the minimal legal stride-2 inputs
    (16, 120, 160, 40, 3, 1),                                         # B = 16 at 120x160: the weight gradient's slab cap binds
]
DW_TOL = 7e-7                # forward / data gradient: k*k-term fp32 sums (measured 2.6e-7)
DW_W_TOL = 3e-7              # weight gradient: sums over B*Ho*Wo pixels (measured 1.0e-7)
_dw_id = lambda c: 'B{}_{}x{}_C{}_k{}s{}'.format(*c)


def _dw_case(B, H, W, C, k, s):
    g = _gen(B * 7919 + H * 131 + W * 17 + C + k * 3 + s)
    Ho, Wo = arch.conv_out(H, k, s), arch.conv_out(W, k, s)
    x = torch.randn(B, H, W, C, generator=g)
    w = torch.randn(C, 1, k, k, generator=g) / k
    dy = torch.randn(B, Ho, Wo, C, generator=g)
    return x, w, dy, Ho, Wo


def _dw_ref(x, w, dy, k, s):
    """float64 autograd of F.conv2d(F.pad(x, static padding), w, stride=s, groups=C): -> out, dx, dw (NHWC / (C,1,k,k))"""
    lo, hi = arch.static_pad(k, s)
    x64 = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    y = F.conv2d(F.pad(x64, (lo, hi, lo, hi)), w64, stride=s, groups=x.shape[3])
    y.backward(dy.double().permute(0, 3, 1, 2))
    return y.detach().permute(0, 2, 3, 1), x64.grad.permute(0, 2, 3, 1), w64.grad


@pytest.mark.parametrize('case', DW_CASES, ids=_dw_id)
def test_depthwise_forward_and_data_gradient_vs_fp64(case):
    """cosy_dw_train_forward (dw_rows_kernel, all four (k, s)) and the data gradient -- cosy_dw_train_backward_data (no add: the
    flipped-tap form at stride 1, dw_bwd_data_kernel at stride 2) and cosy_dw_train_backward_data_add (the skip's gradient on
    the store, stride 1) -- against float64 autograd of the statically padded F.conv2d.  Measured worst: out 2.3e-7, dx 2.6e-7,
    dx + add 1.8e-7 (bound 7e-7)."""
    te = _te()
    lib, ptr, stream = _abi()
    B, H, W, C, k, s = case
    x, w, dy, Ho, Wo = _dw_case(*case)
    out64, dx64, _ = _dw_ref(x, w, dy, k, s)
    xd, dyd = dev(x), dev(dy)
    wt = dev(w.view(C, k * k).t())
    out = te.dw_forward(xd, wt, B, H, W, C, k, s)
    report(f'{_dw_id(case)} out', rel(out.view(B, Ho, Wo, C), out64), DW_TOL)
    dx = torch.full((B, H, W, C), float('nan'), device='cuda')
    assert lib.cosy_dw_train_backward_data(ptr(dyd), ptr(wt), B, H, W, C, k, s, ptr(dx), stream()) == COSY_OK
    report(f'{_dw_id(case)} dx', rel(dx, dx64), DW_TOL)
    if s == 1:
        add = torch.randn(B, H, W, C, generator=_gen(C))
        dxa, _ = te.dw_backward(xd, dyd, wt, B, H, W, C, k, s, add=dev(add))
        report(f'{_dw_id(case)} dx + add', rel(dxa.view(B, H, W, C), dx64 + add.double()), DW_TOL)


@pytest.mark.parametrize('case', DW_CASES, ids=_dw_id)
def test_depthwise_weight_gradient_vs_fp64(case):
    """cosy_dw_train_backward_weight_ex (dw_bwd_weight_kernel: 4-pixel runs, slabs, fixed-order combine) in both layouts --
    module_layout 1 = the module's (C, 1, k, k) (what train_engine.dw_backward asks for), 0 = [tap][C] -- against float64
    autograd; the two layouts are transposes of each other bit for bit; bit-identical re-run.  Measured worst: 1.0e-7 (bound 3e-7)."""
    te = _te()
    lib, ptr, stream = _abi()
    B, H, W, C, k, s = case
    x, w, dy, Ho, Wo = _dw_case(*case)
    _, _, dw64 = _dw_ref(x, w, dy, k, s)
    xd, dyd = dev(x), dev(dy)
    wt = dev(w.view(C, k * k).t())
    _, dw1 = te.dw_backward(xd, dyd, wt, B, H, W, C, k, s)
    report(f'{_dw_id(case)} dw', rel(dw1, dw64), DW_W_TOL)
    dw0 = torch.full((k * k, C), float('nan'), device='cuda')
    ws = te._workspace(xd.device)
    assert lib.cosy_dw_train_backward_weight_ex(ptr(xd), ptr(dyd), B, H, W, C, k, s, ptr(dw0), 0, ptr(ws), stream()) == COSY_OK
    assert torch.equal(dw0.t().reshape(C, 1, k, k), dw1)
    dw0b = torch.full((k * k, C), float('nan'), device='cuda')
    assert lib.cosy_dw_train_backward_weight(ptr(xd), ptr(dyd), B, H, W, C, k, s, ptr(dw0b), ptr(ws), stream()) == COSY_OK
    assert torch.equal(dw0b, dw0)


# ---------------------------------------------------------------------------------------------------------------------------
# per-sample row reductions / broadcasts
# ---------------------------------------------------------------------------------------------------------------------------
ROWS_TOL = 2e-7              # means / dots: double sums, one fp32 rounding (measured 8.1e-8)
ROWS_EW_TOL = 2e-7           # broadcast / scale: elementwise (measured 7.5e-8)
ROWS_CASES = [(1, 1, 4), (3, 129, 68), (16, 19200, 40), (64, 70, 1536), (17, 4096, 144)]


@pytest.mark.parametrize('B,HW,C', ROWS_CASES)
def test_row_reductions_vs_fp64(B, HW, C):
    """cosy_rows_mean, cosy_rows_dot (never called by the step: only its _bn form is), cosy_rows_broadcast, cosy_rows_scale with
    and without add, over (B, HW, C) from one pixel to 16 x 19200 rows; (64, 70, 1536) is where rows_chunks drops to one chunk
    per sample.  Bit-identical re-runs of both reductions.  Measured worst: mean 8.1e-8, dot 4.3e-8 (bound 2e-7); broadcast
    5.2e-8, scale 4.2e-8, scale + add 7.5e-8 (bound 2e-7)."""
    te = _te()
    g = _gen(B * 1000 + HW + C)
    a, a2 = torch.randn(B * HW, C, generator=g) + 0.5, torch.randn(B * HW, C, generator=g) + 0.25
    v, gg, add = torch.randn(B, C, generator=g), torch.randn(B, C, generator=g), torch.randn(B, C, generator=g)
    ad, a2d = dev(a), dev(a2)
    tag = f'B={B} HW={HW} C={C}'
    mean = te.rows_mean(ad, B, HW, C)
    report(tag + ' mean', rel(mean, a.double().view(B, HW, C).mean(1)), ROWS_TOL)
    dot = te.rows_dot(ad, a2d, B, HW, C)
    report(tag + ' dot', rel(dot, (a.double() * a2.double()).view(B, HW, C).sum(1)), ROWS_TOL)
    assert torch.equal(te.rows_mean(ad, B, HW, C), mean) and torch.equal(te.rows_dot(ad, a2d, B, HW, C), dot)
    scale = f32(1.0 / HW)
    rep = lambda t: t.double().repeat_interleave(HW, 0)
    report(tag + ' broadcast', rel(te.rows_broadcast(dev(v), scale, B, HW, C), rep(v) * scale), ROWS_EW_TOL)
    report(tag + ' scale', rel(te.rows_scale(ad, dev(gg), B, HW, C), a.double() * rep(gg)), ROWS_EW_TOL)
    report(tag + ' scale + add', rel(te.rows_scale(ad, dev(gg), B, HW, C, add=dev(add), add_scale=scale),
                                     a.double() * rep(gg) + rep(add) * scale), ROWS_EW_TOL)


# ---------------------------------------------------------------------------------------------------------------------------
# elementwise activations
# ---------------------------------------------------------------------------------------------------------------------------
ACT_FWD_TOL = 4e-7           # per element: |kernel - float64| / max(|float64|, 1) (measured 1.5e-7)
ACT_BWD_TOL = 2e-6           # the same; swish' = s (1 + x (1 - s)) cancels near x = -1.28 (measured 9.3e-7)
SPECIAL = [20.0, -20.0, 88.0, -88.0, 89.0, -89.0, 100.0, -100.0, 1e4, -1e4, 0.0, -0.0]     # expf(-x) overflows beyond 88.7


@pytest.mark.parametrize('n', [1, 255, 257, 1000003])
def test_activations_vs_fp64(n):
    """cosy_act_forward / cosy_act_backward (never called by the step), kind 0 = swish and 1 = sigmoid, against float64 and its
    autograd: n around the 256-thread workgroup; |x| = 20, 88, 89 (expf overflows), 100, 1e4 and +-0 among the inputs.  The
    kernel is finite wherever float64 is; a NaN input gives NaN.  Measured worst: forward 1.5e-7 (bound 4e-7), backward 9.3e-7
    (bound 2e-6)."""
    te = _te()
    g = _gen(n)
    x = torch.randn(n, generator=g) * 4
    if n == 1:
        x[0] = -89.0
    else:
        m = min(n, len(SPECIAL))
        x[:m] = torch.tensor(SPECIAL[:m])
        x[-1] = float('nan')
    dy = torch.randn(n, generator=g)
    xd, dyd = dev(x), dev(dy)
    ok = ~torch.isnan(x)
    for kind, f in ((0, lambda t: t * torch.sigmoid(t)), (1, torch.sigmoid)):
        x64 = x.double().requires_grad_(True)
        y64 = f(x64)
        y64.backward(dy.double())
        for what, got, want in (('forward', te.act_forward(xd, kind).cpu(), y64.detach()), ('backward', te.act_backward(xd, dyd, kind).cpu(), x64.grad)):
            assert torch.isnan(got[~ok]).all(), (kind, what)
            g_, w_ = got[ok].double(), want[ok]
            assert torch.isfinite(g_).all() and torch.isfinite(w_).all()
            err = float(((g_ - w_).abs() / w_.abs().clamp(min=1.0)).max())
            report(f'n={n} kind={kind} {what}', err, ACT_FWD_TOL if what == 'forward' else ACT_BWD_TOL)


# ---------------------------------------------------------------------------------------------------------------------------
# stem im2col
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B,H,W', [(2, 240, 320), (1, 7, 9), (1, 2, 2), (3, 17, 30)])
def test_stem_im2col_bit_exact(B, H, W):
    """cosy_stem_im2col (ld 54, never called by the step) and cosy_stem_im2col_ld (ld 56): bit-exact against F.unfold of the 6-channel
    input padded (0, 1) (the static padding of k 3 s 2), stride 2, in column order (ky*3 + kx)*6 + c.  Channels 6 and 7 of the NHWC8
    input are NaN and `cols` starts as NaN: nothing leaks in, the padding columns 54 .. ld-1 are exactly 0."""
    lib, ptr, stream = _abi()
    x8 = torch.randn(B, H, W, 8, generator=_gen(H * W + B))
    x8[..., 6:] = float('nan')
    Ho, Wo = arch.conv_out(H, 3, 2), arch.conv_out(W, 3, 2)
    lo, hi = arch.static_pad(3, 2)
    u = F.unfold(F.pad(x8[..., :6].permute(0, 3, 1, 2), (lo, hi, lo, hi)), 3, stride=2)          # (B, c*9 + tap, Ho*Wo)
    want = u.view(B, 6, 9, Ho * Wo).permute(0, 3, 2, 1).reshape(B * Ho * Wo, 54)
    xd = dev(x8)
    for ld in (54, 56):
        cols = torch.full((B * Ho * Wo, ld), float('nan'), device='cuda')
        rc = lib.cosy_stem_im2col(ptr(xd), B, H, W, ptr(cols), stream()) if ld == 54 else \
            lib.cosy_stem_im2col_ld(ptr(xd), B, H, W, ld, ptr(cols), stream())
        assert rc == COSY_OK
        got = cols.cpu()
        assert not torch.isnan(got).any(), ld
        assert torch.equal(got[:, :54], want), ld
        assert (got[:, 54:] == 0).all(), ld


# ---------------------------------------------------------------------------------------------------------------------------
# gradient of the disentangled loss
# ---------------------------------------------------------------------------------------------------------------------------
LOSS_TOL = 4e-7              # per row: max |kernel - float64| / max |float64| of that row (measured 1.6e-7)
LOSS_CASES = [(1, 1, 1, False), (1, 5, 257, True), (64, 2, 255, False), (64, 5, 256, True), (64, 1, 2600, True), (64, 2, 2600, False)]
MARGIN = 1e-4                # every residual and every best / second-best gap is at least this, relative


def _rot(rs, angle):
    axis = rs.randn(3)
    axis /= np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(angle) * Kx + (1 - math.cos(angle)) * Kx @ Kx


def _loss_preds(gt, TCO, out9, K):
    """the three predicted poses of loss_refiner_CO_disentangled (rotation / image-plane translation / depth terms), float64"""
    from cosy_oracle import TorchRef
    dR = TorchRef.ortho6d(out9[:, :6], torch)
    g0 = gt[:, 0]
    orn = g0.clone(); orn[:, :3, :3] = dR @ TCO[:, :3, :3]
    xy = g0.clone()
    xy[:, :2, 3] = (out9[:, 6:8] / K[:, [0, 1], [0, 1]] + TCO[:, :2, 3] / TCO[:, 2:3, 3]) * g0[:, 2:3, 3]
    zz = g0.clone(); zz[:, 2, 3] = out9[:, 8] * TCO[:, 2, 3]
    return orn, xy, zz


def _xform(T, p):
    """T (..., 4, 4) applied to the points p (..., P, 3), elementwise (no BLAS: equal rows give equal coordinates) -> (..., P, 3)"""
    return torch.stack([T[..., r, None, 0] * p[..., 0] + T[..., r, None, 1] * p[..., 1] + T[..., r, None, 2] * p[..., 2] + T[..., r, None, 3]
                        for r in range(3)], -1)


def _residuals(pred, gt, pts):
    """pred (B,4,4), gt (B,S,4,4), pts (B,P,3) -> (B,S,P,3) transformed-point differences"""
    return _xform(pred, pts).unsqueeze(1) - _xform(gt, pts.unsqueeze(1))


def _loss_case(B, S, P, table, seed):
    rs = np.random.RandomState(seed)
    TCO = np.tile(np.eye(4), (B, 1, 1))
    gt = np.tile(np.eye(4), (B, S, 1, 1))
    out9 = np.zeros((B, 9))
    K = np.tile(np.eye(3), (B, 1, 1))
    for b in range(B):
        R0 = _rot(rs, rs.uniform(0, math.pi))
        TCO[b, :3, :3] = R0
        TCO[b, :3, 3] = [rs.randn() * 0.05, rs.randn() * 0.05, 0.8 + rs.randn() * 0.1]
        dR = _rot(rs, rs.uniform(0.05, 0.3))
        for s in range(S):
            gt[b, s, :3, :3] = _rot(rs, rs.uniform(0.05, 0.3) * (1 + s)) @ R0
            gt[b, s, :3, 3] = TCO[b, :3, 3] + rs.randn(3) * 0.02 * (1 + s)
            if s and rs.rand() < 0.5:       # a later ground truth near the predicted rotation: the argmin picks it for some terms
                gt[b, s, :3, :3] = _rot(rs, rs.uniform(0.03, 0.08)) @ dR @ R0
                gt[b, s, :3, 3] = gt[b, 0, :3, 3] + rs.randn(3) * 0.004
        out9[b, :6] = np.concatenate([dR[:, 0], dR[:, 1] * rs.uniform(0.5, 2.0) + dR[:, 0] * rs.uniform(-0.3, 0.3)])
        K[b, 0, 0], K[b, 1, 1] = rs.uniform(300, 600), rs.uniform(300, 600)
        K[b, :2, 2] = [rs.uniform(100, 200), rs.uniform(100, 200)]
        # image-plane and depth outputs that miss the first ground truth by 5 - 20 mm (random sign): no residual near 0
        miss = rs.uniform(0.005, 0.02, 3) * rs.choice([-1, 1], 3)
        zg, zi = gt[b, 0, 2, 3], TCO[b, 2, 3]
        out9[b, 6:8] = ((gt[b, 0, :2, 3] + miss[:2]) / zg - TCO[b, :2, 3] / zi) * K[b, [0, 1], [0, 1]]
        out9[b, 8] = (zg + miss[2]) / zi
    # fp32 inputs (what the kernel gets); the float64 reference starts from the same values
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))
    gt, TCO, out9, K = T(gt), T(TCO), T(out9), T(K)
    n_obj = max(B * 5 // 8, 1) if table else B
    obj = torch.from_numpy((rs.permutation(B) % n_obj).astype(np.int32)) if table else torch.arange(B, dtype=torch.int32)
    preds = _loss_preds(gt.double(), TCO.double(), out9.double(), K.double())
    # points: oversampled per object, kept where every residual against every ground truth of every row that uses the object is
    # >= MARGIN of that row's coordinate scale (or exactly 0: a coordinate the term copies from the ground truth)
    cand = torch.from_numpy(rs.uniform(-0.1, 0.1, (n_obj, 16 * P + 64, 3)).astype(np.float32))
    keep = torch.ones(n_obj, cand.shape[1], dtype=torch.bool)
    for b in range(B):
        o = int(obj[b])
        pb = cand[o].double()[None]
        scale = float(_xform(gt.double()[b, 0], pb[0]).abs().max())
        for pred in preds:
            r = _residuals(pred[b:b + 1], gt.double()[b:b + 1], pb)[0].abs()    # (S, Pc, 3)
            keep[o] &= ((r == 0) | (r >= MARGIN * scale)).all(-1).all(0)
    pts = torch.stack([cand[o][keep[o]][:P] for o in range(n_obj)])
    assert pts.shape == (n_obj, P, 3), 'not enough candidate points: change the seed'
    dloss = torch.from_numpy(np.where(np.arange(B) % 4 == 3, 0.0, rs.randn(B)).astype(np.float32))
    return gt, TCO, out9, K, pts, obj, dloss


@pytest.mark.parametrize('B,S,P,table', LOSS_CASES)
def test_loss_disentangled_backward_vs_fp64(oracle, B, S, P, table):
    """cosy_loss_refiner_disentangled_backward (per-row points, and the pts_table + obj_id form the step never uses) against float64
    autograd of TorchRef.disentangled_loss times a per-row dloss with zeros.  The test first asserts that every residual
    |pred - gt| of the assigned ground truth and every gap between the best and second-best ground truth is >= 1e-4 relative,
    so that no sign flip or tie can be the cause of a failure.  S = 1: the same call with the ground truth given twice (S = 2)
    is the same bit for bit.  Measured worst: 1.6e-7 (bound 4e-7)."""
    lib, ptr, stream = _abi()
    gt, TCO, out9, K, pts, obj, dloss = _loss_case(B, S, P, table, seed=B * 100 + S * 10 + P)
    rows_pts = pts[obj.long()].double()
    # preconditions, on the points actually used
    for b in range(B):
        scale = float(_xform(gt.double()[b, 0], rows_pts[b]).abs().max())
        for t, pred in enumerate(_loss_preds(gt.double(), TCO.double(), out9.double(), K.double())):
            r = _residuals(pred[b:b + 1], gt.double()[b:b + 1], rows_pts[b:b + 1])[0]
            d = r.abs().mean((1, 2))
            srt = torch.sort(d).values
            assert S == 1 or float(srt[1] - srt[0]) >= MARGIN * float(srt[0]), (b, t, srt)
            rb = r[int(d.argmin())].abs()
            assert bool(((rb == 0) | (rb >= MARGIN * scale)).all()), (b, t)
    out64 = out9.double().requires_grad_(True)
    loss = oracle.TorchRef({}).disentangled_loss(gt.double(), TCO.double(), out64, K.double(), rows_pts)
    (loss * dloss.double()).sum().backward()

    def kernel(gt_, S_):
        d = torch.full((B, 9), float('nan'), device='cuda')
        g_, t_, o_, k_, p_, dl_ = dev(gt_), dev(TCO), dev(out9), dev(K), dev(pts), dev(dloss)
        ob = dev(obj) if table else None
        rc = lib.cosy_loss_refiner_disentangled_backward(ptr(g_), ptr(t_), ptr(o_), ptr(k_), ptr(p_), ptr(ob), B, S_, P, ptr(dl_), ptr(d), stream())
        assert rc == COSY_OK
        return d.cpu()

    got = kernel(gt, S)
    want = out64.grad
    err = float(((got.double() - want).abs().max(1).values / want.abs().max(1).values.clamp(min=1e-30)).max())
    assert torch.equal(got[dloss == 0], torch.zeros_like(got[dloss == 0]))
    report(f'B={B} S={S} P={P} table={int(table)} d_refiner_outputs', err, LOSS_TOL)
    if S == 1:
        assert torch.equal(kernel(torch.cat([gt, gt], 1), 2), got)


# ---------------------------------------------------------------------------------------------------------------------------
# gradient-norm clip + Adam
# ---------------------------------------------------------------------------------------------------------------------------
NORM_TOL = 1e-7              # total norm: double sum of squares, fp32 result (measured 3.6e-8)
COEF_TOL = 2e-7              # the clip coefficient, from the fp32 norm (measured 7.8e-8)
ADAM_TOL = 5e-7              # exp_avg / exp_avg_sq after every step (measured 1.9e-7)
LR, BETAS, EPS = f32(3e-4), (f32(0.9), f32(0.999)), f32(1e-8)


def _ulp32(a):
    return torch.from_numpy(np.spacing(np.abs(a.numpy()).astype(np.float32))).double()


def _adam_param_excess(p, p64, t, lr, cond=0.0):
    """max over elements of |p - p64| / (t ulp(p) + 1e-4 lr t + cond): < 1 when every element is inside the trajectory bound"""
    allowed = t * _ulp32(p64) + 1e-4 * lr * t + cond
    return float(((p.double() - p64).abs() / allowed).max())


@pytest.mark.parametrize('n,max_norm,wd', [(1, 0.5, 0.0), (257, 0.0, 1e-2), (257, 0.5, 1e-2), (1000003, 1e9, 0.0), (1000003, 0.5, 1e-2)])
def test_grad_norm_clip_and_adam_vs_torch_fp64(n, max_norm, wd):
    """cosy_grad_norm_clip (max_norm 0 = off, 0.5 = active, 1e9 = inactive) and cosy_adam_step (weight decay 0 / 1e-2) for 10
    consecutive steps with fresh gradients (some exactly 0, and one step entirely 0), against torch.nn.utils.clip_grad_norm_ +
    torch.optim.Adam on float64 copies with the same fp32 hyperparameters: the norm; the coefficient min(1, max_norm / (norm + 1e-6));
    m and v; the parameters after step t within t ulp(p) + 1e-4 lr t of the float64 trajectory, plus, per element, the fp32 rounding
    of the clipped, decayed gradient c g + wd p (one ulp of |c g| + |wd p|) times the update's gain lr / (sqrt(v_hat) + eps), summed over
    the steps: where c g and wd p cancel to about eps (n = 10^6, clip and decay both on), an exact fp32 evaluation of Adam is already
    5.9x outside the bare bound.  Bit-identical re-run of the norm.  Measured worst: norm 3.6e-8 (bound 1e-7), coefficient 7.8e-8
    (bound 2e-7), m 1.6e-7 and v 1.9e-7 (bound 5e-7), parameters 0.49 of their allowance (bound 1)."""
    te = _te()
    lib, ptr, stream = _abi()
    g = _gen(n + int(max_norm * 10) + int(wd * 1e4))
    wd = f32(wd)
    p0 = torch.randn(n, generator=g)
    p64 = torch.nn.Parameter(p0.double().clone())
    opt = torch.optim.Adam([p64], lr=LR, betas=BETAS, eps=EPS, weight_decay=wd)
    pd, md, vd = dev(p0), torch.zeros(n, device='cuda'), torch.zeros(n, device='cuda')
    nc, nc2 = torch.empty(2, device='cuda'), torch.empty(2, device='cuda')
    ws = te._workspace(pd.device)
    worst = dict(norm=0.0, coef=0.0, m=0.0, v=0.0, p=0.0)
    cond = torch.zeros(n, dtype=torch.float64)
    for t in range(1, 11):
        gr = torch.randn(n, generator=g) * 2
        gr[torch.rand(n, generator=g) < 0.1] = 0.0
        if t == 4:
            gr.zero_()
        gd = dev(gr)
        assert lib.cosy_grad_norm_clip(ptr(gd), n, max_norm, ptr(nc), ptr(ws), stream()) == COSY_OK
        assert lib.cosy_grad_norm_clip(ptr(gd), n, max_norm, ptr(nc2), ptr(ws), stream()) == COSY_OK
        assert torch.equal(nc, nc2)
        p64.grad = gr.double()
        if max_norm > 0:
            norm64 = float(torch.nn.utils.clip_grad_norm_([p64], max_norm))
            coef64 = min(1.0, max_norm / (norm64 + 1e-6))
        else:
            norm64, coef64 = float(p64.grad.norm()), 1.0
        delta = _ulp32((coef64 * gr.double()).abs() + wd * p64.detach().abs())        # fp32 rounding of c g + wd p
        assert lib.cosy_adam_step(ptr(pd), ptr(gd), ptr(md), ptr(vd), n, LR, BETAS[0], BETAS[1], EPS, wd, t, ptr(nc), stream()) == COSY_OK
        opt.step()
        st = opt.state[p64]
        cond += LR * delta / ((st['exp_avg_sq'] / (1 - BETAS[1] ** t)).sqrt() + EPS)
        nch = nc.cpu().double()
        worst['norm'] = max(worst['norm'], abs(float(nch[0]) - norm64) / max(norm64, 1e-30) if norm64 else abs(float(nch[0])))
        worst['coef'] = max(worst['coef'], abs(float(nch[1]) - coef64) / coef64)
        worst['m'] = max(worst['m'], rel(md, st['exp_avg']))
        worst['v'] = max(worst['v'], rel(vd, st['exp_avg_sq']))
        worst['p'] = max(worst['p'], _adam_param_excess(pd.cpu(), p64.detach(), t, LR, cond))
    tag = f'n={n} max_norm={max_norm:g} wd={wd:g}'
    report(tag + ' norm', worst['norm'], NORM_TOL)
    report(tag + ' coef', worst['coef'], COEF_TOL)
    report(tag + ' exp_avg', worst['m'], ADAM_TOL)
    report(tag + ' exp_avg_sq', worst['v'], ADAM_TOL)
    report(tag + ' params / allowance', worst['p'], 1.0)


def test_flat_adam_vs_torch_fp64():
    """train_engine.FlatAdam (flat buffers, clip_grad_norm 0.5, weight decay 1e-2) on a small module whose parameter sizes are not
    multiples of 4 (35, 5, 15, 3), 5 steps with fresh gradients: the same parameters as torch's clip_grad_norm_ + Adam in float64
    (within t ulp(p) + 1e-4 lr t), and the returned norm.  Measured worst: norm 2.4e-8 (bound 1e-7), parameters 0.21 of their
    allowance (bound 1)."""
    te = _te()
    g = _gen(11)
    torch.manual_seed(11)
    model = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Tanh(), torch.nn.Linear(5, 3))
    ref = [torch.nn.Parameter(p.detach().double().clone()) for p in model.parameters()]
    model = model.cuda()
    wd = f32(1e-2)
    opt = te.FlatAdam(model, lr=LR, betas=BETAS, eps=EPS, weight_decay=wd, clip_grad_norm=0.5)
    ropt = torch.optim.Adam(ref, lr=LR, betas=BETAS, eps=EPS, weight_decay=wd)
    worst_norm = worst_p = 0.0
    for t in range(1, 6):
        opt.zero_grad()
        grads = []
        for p in model.parameters():
            gr = torch.randn(p.shape, generator=g)
            gr[torch.rand(p.shape, generator=g) < 0.2] = 0.0
            grads.append(gr)
            p.grad.copy_(gr)
        norm = float(opt.step())
        for q, gr in zip(ref, grads):
            q.grad = gr.double()
        norm64 = float(torch.nn.utils.clip_grad_norm_(ref, 0.5))
        ropt.step()
        worst_norm = max(worst_norm, abs(norm - norm64) / norm64)
        for p, q in zip(model.parameters(), ref):
            worst_p = max(worst_p, _adam_param_excess(p.detach().cpu(), q.detach(), t, LR))
    report('FlatAdam norm', worst_norm, NORM_TOL)
    report('FlatAdam params / (t ulp + 1e-4 lr t)', worst_p, 1.0)


# ---------------------------------------------------------------------------------------------------------------------------
# argument contract
# ---------------------------------------------------------------------------------------------------------------------------
def test_argument_contract_c_multiple_of_4_and_stride2_one_pixel():
    """(1) cosy_bn_train_stats, cosy_rows_mean and cosy_rows_dot read 16-byte channel quads: C % 4 != 0 is COSY_EINVAL.
    (2) Stride 2 with a 1-pixel side has no output under the static padding (arch.conv_out(1, k, 2) == 0): the depthwise
    forward and both gradients refuse it.  cosy_last_error() names the offending value, the outputs are untouched.
    Harmless even where a guard is missing: case (1) is one row of C = 6 in buffers of 16 floats (the quad loads stay aligned
    and inside them), case (2) sizes every buffer for the 1-row output C's truncating division would give."""
    te = _te()
    lib, ptr, stream = _abi()
    SENT = 1234.5
    ws = te._workspace('cuda')

    def expect_einval(rc, names, *outs):
        msg = lib.cosy_last_error().decode()
        assert rc == COSY_EINVAL, (rc, msg)
        for s in names:
            assert s in msg, (s, msg)
        for o in outs:
            assert (o == SENT).all(), msg

    buf = lambda n: torch.full((n,), SENT, device='cuda')
    x, x2 = torch.randn(16, device='cuda'), torch.randn(16, device='cuda')
    mean, rstd, rm, rv = buf(16), buf(16), buf(16), buf(16)
    expect_einval(lib.cosy_bn_train_stats(ptr(x), 1, 6, BN_EPS, BN_MOM, ptr(mean), ptr(rstd), ptr(rm), ptr(rv), ptr(ws), stream()),
                  ['C=6'], mean, rstd, rm, rv)
    out = buf(16)
    expect_einval(lib.cosy_rows_mean(ptr(x), 1, 1, 6, ptr(out), ptr(ws), stream()), ['C=6'], out)
    expect_einval(lib.cosy_rows_dot(ptr(x), ptr(x2), 1, 1, 6, ptr(out), ptr(ws), stream()), ['C=6'], out)
    torch.cuda.synchronize()
    B, C = 1, 4
    for H, W in ((1, 5), (5, 1), (1, 1)):
        for k in (3, 5):
            Hc, Wc = int((H - 2) / 2) + 1, int((W - 2) / 2) + 1      # C's truncating division: 1 for a 1-pixel side
            names = [f'H={H}', f'W={W}']
            xin, dy, wt, add = (torch.randn(n, device='cuda') for n in (B * H * W * C, B * Hc * Wc * C, k * k * C, B * H * W * C))
            y, dx, dw = buf(B * Hc * Wc * C), buf(B * H * W * C), buf(k * k * C)
            expect_einval(lib.cosy_dw_train_forward(ptr(xin), ptr(wt), B, H, W, C, k, 2, ptr(y), stream()), names, y)
            expect_einval(lib.cosy_dw_train_backward_data(ptr(dy), ptr(wt), B, H, W, C, k, 2, ptr(dx), stream()), names, dx)
            expect_einval(lib.cosy_dw_train_backward_data_add(ptr(dy), ptr(wt), None, B, H, W, C, k, 2, ptr(dx), stream()), names, dx)
            expect_einval(lib.cosy_dw_train_backward_weight(ptr(xin), ptr(dy), B, H, W, C, k, 2, ptr(dw), ptr(ws), stream()), names, dw)
            for layout in (0, 1):
                expect_einval(lib.cosy_dw_train_backward_weight_ex(ptr(xin), ptr(dy), B, H, W, C, k, 2, ptr(dw), layout, ptr(ws), stream()),
                              names, dw)
    torch.cuda.synchronize()
