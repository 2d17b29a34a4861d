"""The training step's matrix-pipe kernels (v_mfma_f32_16x16x4_f32), each held on its own: cosy_train_gemm / cosy_train_gemm_packed
with cosy_train_pack_plan / _pack_all (the fp32 pw_gemm_dma tiles of csrc/kernels_net.hip), cosy_wgrad (wgrad_tall_kernel<TN,TK> and the
combine_partials_kernel<float> pass behind it), cosy_se_train_forward / _backward, cosy_fc_small_forward / _backward, and the
on-the-fly row reductions cosy_rows_mean_bn / cosy_rows_dot_bn (csrc/kernels_train.hip).

Three kinds of check, all against float64 products formed with stock torch on the CPU from the fp32 operands the kernel gets:
  1. EXACT: operands are integers in [-8, 8] stored as fp32.  Every product is an integer of magnitude <= 64 and every partial sum
     in any order stays below 2^24 (asserted per case), so fp32 arithmetic is exact whatever the order: the kernel must return the
     float64 product bit for bit (torch.equal, no tolerance).  A tail mask that drops or doubles a row, a wrong fragment index, a slab
     added twice are each off by >= 1.
  2. GAUSSIAN: a length-n fp32 sum of products in ANY order obeys |got - want| <= gamma_n (|A| |B|) elementwise, gamma_n = n u / (1 - n u),
     u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, eq. 3.5): every term passes through one product rounding and at
     most n - 1 additions.  n = the reduction length plus what the kernel adds behind it: one for the `add` operand or a bias, one for
     the fp32 rounding of the weight gradient's float64 combine.  Bound and reference come from the operands, never from the kernel.
  3. LIMITS: squeeze-excite, fc_small and rows_*_bn at the edges of what their entry points admit, against float64 autograd, with the
     bounds test_gpu_parity.py::test_se_train_kernels_vs_torch_fp64 uses (2e-6 forward, 5e-6 gradients and row reductions).
and the argument contract by return code.  Every case prints its measured figures (-s).
"""
import ctypes

import pytest
import torch

from test_train_kernels import COSY_EINVAL, COSY_OK, _abi, _gen, _te, dev, rel, report

pytestmark = pytest.mark.gpu

U = 2.0 ** -24               # unit roundoff of fp32
cdiv = lambda a, b: -(-a // b)


def gamma(n):
    assert n * U < 1
    return n * U / (1.0 - n * U)


def ints(g, *shape):
    """integers in [-8, 8] as fp32"""
    return torch.randint(-8, 9, shape, generator=g).float()


def assert_exact_range(a, b, length, *added):
    """the precondition of every bit-equality check: no partial sum of `length` products a b (plus the added terms) can reach 2^24"""
    top = float(a.abs().max()) * float(b.abs().max()) * length + sum(float(t.abs().max()) for t in added)
    assert top < 2 ** 24, top


def assert_within(tag, got, want64, absprod64, n):
    """|got - want| <= gamma_n * (|A| |B|) elementwise; prints the worst ratio of error to bound"""
    err = (got.detach().cpu().double() - want64).abs()
    bound = gamma(n) * absprod64
    assert bool((bound[err > 0] > 0).all()), tag
    ratio = float((err / bound.clamp(min=1e-300)).max())
    print(f'  {tag}: worst error / bound = {ratio:.3g} (gamma_{n} = {gamma(n):.3g})')
    assert bool((err <= bound).all()), (tag, ratio)
    return ratio


# ---------------------------------------------------------------------------------------------------------------------------
# cosy_wgrad: which kernel a shape reaches, restated from cosy_wgrad's own launch arithmetic
# ---------------------------------------------------------------------------------------------------------------------------
WG_CAP = 256                 # workgroups along M (the library's default; the tuning knob exists in the experiment build only)
WGRAD_INSTANCES = {(3, 1), (3, 2), (3, 3), (3, 4), (2, 1), (2, 2), (2, 3), (2, 4), (2, 9), (2, 12)}      # what cosy_wgrad dispatches


def wgrad_plan(M, N, K, workspace_bytes):
    """-> (TN, TK, gy, gz, rows per wave, slabs) as cosy_wgrad chooses them"""
    tk, tn = cdiv(K, 16), cdiv(N, 16)
    TN = 3 if tn % 3 == 0 and tk <= 4 else 2
    TK = tk if tk <= 4 else tk if tk in (9, 12) and N * K <= 192 * 192 else 4
    gy, gz = cdiv(tn, TN), cdiv(tk, TK)
    cap = workspace_bytes // (N * K * 4)
    assert cap >= 1
    nwg = min(WG_CAP, cap)
    if gy * gz >= 64:
        nwg = min(nwg, 64)
    rpw = cdiv(cdiv(M, nwg * 4), 8) * 8
    return TN, TK, gy, gz, rpw, cdiv(M, rpw * 4)


def _ws_bytes():
    lib, _, _ = _abi()
    return int(lib.cosy_train_workspace_bytes())


# (M, N, K) -> the instantiation <TN,TK> it selects (asserted against wgrad_plan) and, where it matters, (gy, gz)
WGRAD_SHAPES = [
    ((37, 48, 16), (3, 1), None),
    ((37, 33, 5), (3, 1), None),            # ragged N and K (wgrad has no % 4 rule)
    ((37, 96, 24), (3, 2), None),
    ((37, 144, 40), (3, 3), None),
    ((37, 48, 64), (3, 4), None),
    ((37, 24, 8), (2, 1), None),
    ((37, 16, 32), (2, 2), None),
    ((37, 24, 40), (2, 3), None),
    ((37, 32, 64), (2, 4), None),
    ((37, 24, 144), (2, 9), None),          # the project convolution 144 -> 24
    ((37, 48, 132), (2, 9), (2, 1)),        # gy = 2, ragged K
    ((37, 32, 192), (2, 12), None),         # the project convolution 192 -> 32
    ((37, 20, 180), (2, 12), None),
    ((37, 288, 144), (2, 4), (9, 3)),       # tk = 9 but N K > 192^2: TK = 4, gz = 3, the last z-block one tile wide
    ((37, 1024, 80), (2, 4), (32, 2)),      # gy gz = 64: the branch that caps the slabs at 64 (2 slabs at this M)
]
# rows: one or two workgroups, partial 4-row steps, waves without rows (N, K = 24, 40: <2,3>)
WGRAD_M_TAILS = [((M, 24, 40), (2, 3), None) for M in (1, 3, 4, 5, 8, 9, 31, 32, 33)]
# slabs: which loops of combine_partials_kernel run -- (shape, instance, slabs expected, the range that loop structure needs)
WGRAD_SLABS = [
    ((8191, 24, 40), (2, 3), 256, (241, 1 << 30)),      # > 240: the 16-deep loop (every wave once); the last wave has 7 rows
    ((8193, 24, 40), (2, 3), 129, (49, 240)),           # (48, 240]: the 4-deep loop twice, then the tail loop (wave 0)
    ((8191, 1024, 80), (2, 4), 64, (64, 64)),           # the 64-slab cap binds: the 4-deep loop once, no tail
]
NETWORK_MKN = [(4800, 24, 144), (1229, 136, 816), (76800, 40, 24), (333, 384, 1536), (5120, 1392, 232), (64, 56, 40)]   # test_gpu_parity's
WGRAD_NETWORK = [((4800, 144, 24), (3, 2)), ((1229, 816, 136), (2, 4)), ((76800, 24, 40), (2, 3)), ((333, 1536, 384), (2, 4)),
                 ((5120, 232, 1392), (2, 4)), ((64, 40, 56), (3, 4))]
WGRAD_EXACT = [(s, i, g, None, None) for s, i, g in WGRAD_SHAPES + WGRAD_M_TAILS] + [(s, i, None, n, r) for s, i, n, r in WGRAD_SLABS]
WGRAD_GAUSS = WGRAD_EXACT + [(s, i, None, None, None) for s, i in WGRAD_NETWORK]
_wg_id = lambda c: 'M{}_N{}_K{}'.format(*c[0])


def test_wgrad_cases_reach_all_ten_instantiations():
    """The restated selection rule sends the exact-integer cases to every wgrad_tall_kernel<TN,TK> that cosy_wgrad dispatches."""
    ws = _ws_bytes()
    reached = {wgrad_plan(*shape, ws)[:2] for shape, *_ in WGRAD_EXACT}
    assert reached == WGRAD_INSTANCES, sorted(WGRAD_INSTANCES - reached)
    assert {inst for _, inst, *_ in WGRAD_EXACT} == WGRAD_INSTANCES


def _check_wgrad_plan(case):
    (M, N, K), inst, grid, nslab, slab_range = case
    TN, TK, gy, gz, rpw, slabs = wgrad_plan(M, N, K, _ws_bytes())
    assert (TN, TK) == inst, ((TN, TK), inst)
    if grid is not None:
        assert (gy, gz) == grid, ((gy, gz), grid)
    if nslab is not None:
        assert slabs == nslab and slab_range[0] <= slabs <= slab_range[1], (slabs, nslab, slab_range)
    return f'<{TN},{TK}> grid ({slabs},{gy},{gz}) rows/wave {rpw}'


def _run_wgrad(te, dY, X):
    N, K = dY.shape[1], X.shape[1]
    out = torch.full((N, K), float('nan'), device='cuda')
    out2 = torch.full((N, K), float('nan'), device='cuda')
    dYd, Xd = dev(dY), dev(X)
    te.wgrad(dYd, Xd, out=out)
    te.wgrad(dYd, Xd, out=out2)
    assert torch.equal(out, out2)              # fixed-order combine: a second run is the same bit for bit
    return out.cpu()


@pytest.mark.parametrize('case', WGRAD_EXACT, ids=_wg_id)
def test_wgrad_exact_integers(case):
    """cosy_wgrad on integer operands equals the float64 product dY^T X bit for bit, at one shape per instantiation, at M = 1 .. 33
    (partial 4-row MFMA steps, waves whose r0 >= M), and at the slab counts where combine_partials_kernel changes loops."""
    te = _te()
    M, N, K = case[0]
    print('  ' + _check_wgrad_plan(case))
    g = _gen(M * 1009 + N * 31 + K)
    dY, X = ints(g, M, N), ints(g, M, K)
    assert_exact_range(dY, X, M)
    want = (dY.double().t() @ X.double()).float()
    assert torch.equal(_run_wgrad(te, dY, X), want)


@pytest.mark.parametrize('case', WGRAD_GAUSS, ids=_wg_id)
def test_wgrad_gaussian_componentwise_bound(case):
    """cosy_wgrad on Gaussian operands inside gamma_{M+1} (|dY|^T |X|) elementwise: M products summed in fp32 in the kernel's own
    order (MFMA chain per wave, four waves through LDS), the slabs in float64, one rounding to fp32.  Measured worst error / bound:
    0.48 (M = 1: gamma_2), 0.0019 for M > 100 (the bound grows with M, a rounding error with its square root)."""
    te = _te()
    M, N, K = case[0]
    print('  ' + _check_wgrad_plan(case))
    g = _gen(M * 1009 + N * 31 + K + 1)
    dY, X = torch.randn(M, N, generator=g), torch.randn(M, K, generator=g)
    got = _run_wgrad(te, dY, X)
    assert_within(f'wgrad {_wg_id(case)}', got, dY.double().t() @ X.double(), dY.double().abs().t() @ X.double().abs(), M + 1)


# ---------------------------------------------------------------------------------------------------------------------------
# cosy_train_gemm / cosy_train_gemm_packed: the fp32 pw_gemm_dma tiles at their edges
# ---------------------------------------------------------------------------------------------------------------------------
# (M, K, N).  pw_choose_cfg: N = 8, 24 -> 32-column tiles (NI2,WN1); 40 -> 48 (NI3,WN1); 96, 136 -> 96 (NI3,WN2; 136 = one quad pair
# past a 128-column tile, two n-tiles); 128 -> 128 (NI4,WN2).  WN = 1 tiles hold 256 rows, WN = 2 tiles 128.  K: 16 per k-block, the
# count rounded up to even; K <= 32 runs the 2-stage ring, above that 3 stages.
GEMM_EDGE = ([(67, 24, N) for N in (8, 24, 40, 96, 128, 136)] +
             [(67, K, 40) for K in (8, 16, 32, 40, 48, 56)] +
             [(M, 24, N) for N in (128, 40) for M in (1, 127, 128, 129, 255, 256, 257, 1025)])
GEMM_KN = sorted({(K, N) for _, K, N in GEMM_EDGE})
_mkn_id = lambda c: 'M{}_K{}_N{}'.format(*c)
_weights = {}


def _gemm_weights(kind):
    """one weight per (K, N) of GEMM_EDGE and orientation, W (N, K) and W (K, N), made once; -> ({(K, N): (W_nk, W_kn)}, all of them)"""
    if kind not in _weights:
        g = _gen(77 if kind == 'int' else 78)
        make = (lambda *s: ints(g, *s)) if kind == 'int' else (lambda *s: torch.randn(*s, generator=g))
        _weights[kind] = {kn: (dev(make(kn[1], kn[0])), dev(make(kn[0], kn[1]))) for kn in GEMM_KN}
    ws = _weights[kind]
    return ws, [w for pair in ws.values() for w in pair]


def _gemm_calls(te, A, add_n, W_nk, W_kn, packed):
    """the four calls of a case: forward, forward + add, data-gradient orientation, the same + add -> CPU tensors"""
    Ad, addd = dev(A), dev(add_n)
    return [te.gemm(Ad, W_nk, packed=packed).cpu(), te.gemm(Ad, W_nk, add=addd, packed=packed).cpu(),
            te.gemm(Ad, W_kn, w_is_kn=True, packed=packed).cpu(), te.gemm(Ad, W_kn, w_is_kn=True, add=addd, packed=packed).cpu()]


def _gemm_refs(A, add_n, W_nk, W_kn, absolute=False):
    f = (lambda t: t.cpu().double().abs()) if absolute else (lambda t: t.cpu().double())
    fw, kn = f(A) @ f(W_nk).t(), f(A) @ f(W_kn)
    return [fw, fw + f(add_n), kn, kn + f(add_n)]


GEMM_NAMES = ('A.W^T', 'A.W^T + add', 'A.W (w_is_kn)', 'A.W (w_is_kn) + add')


@pytest.mark.parametrize('case', GEMM_EDGE, ids=_mkn_id)
def test_gemm_exact_integers(case):
    """cosy_train_gemm in both orientations, with and without `add`, on integer operands: the float64 product bit for bit; and
    cosy_train_gemm_packed, from ONE PackedWeights that holds every weight of GEMM_EDGE in both orientations, the same again."""
    te = _te()
    M, K, N = case
    ws, every = _gemm_weights('int')
    W_nk, W_kn = ws[(K, N)]
    g = _gen(M * 1009 + K * 31 + N)
    A, add = ints(g, M, K), ints(g, M, N)
    assert_exact_range(A, W_nk, K, add)
    assert_exact_range(A, W_kn, K, add)
    want = [t.float() for t in _gemm_refs(A, add, W_nk, W_kn)]
    pk = te.PackedWeights.current(every)
    for name, w, got, gotp in zip(GEMM_NAMES, want, _gemm_calls(te, A, add, W_nk, W_kn, None), _gemm_calls(te, A, add, W_nk, W_kn, pk)):
        assert torch.equal(got, w), name
        assert torch.equal(gotp, w), name + ' packed'


def _gemm_gaussian(te, M, K, N, W_nk, W_kn, packed):
    g = _gen(M * 1009 + K * 31 + N + 1)
    A, add = torch.randn(M, K, generator=g), torch.randn(M, N, generator=g)
    want, absprod = _gemm_refs(A, add, W_nk, W_kn), _gemm_refs(A, add, W_nk, W_kn, absolute=True)
    got = _gemm_calls(te, A, add, W_nk, W_kn, None)
    for i, name in enumerate(GEMM_NAMES):
        assert_within(f'gemm M={M} K={K} N={N} {name}', got[i], want[i], absprod[i], K + (i & 1))    # K products (+ the add)
    if packed is not None:
        for name, a, b in zip(GEMM_NAMES, got, _gemm_calls(te, A, add, W_nk, W_kn, packed)):
            assert torch.equal(a, b), name + ': packed != per-call'


@pytest.mark.parametrize('case', GEMM_EDGE, ids=_mkn_id)
def test_gemm_gaussian_componentwise_bound(case):
    """cosy_train_gemm on Gaussian operands inside gamma_K (|A| |W|) elementwise (gamma_{K+1} (|A| |W| + |add|) with `add`), both
    orientations; the packed form equals the per-call form bit for bit.  Measured worst error / bound: 0.30 without add, 0.32 with
    (K = 8)."""
    te = _te()
    M, K, N = case
    ws, every = _gemm_weights('gauss')
    _gemm_gaussian(te, M, K, N, *ws[(K, N)], te.PackedWeights.current(every))


@pytest.mark.parametrize('case', NETWORK_MKN, ids=_mkn_id)
def test_gemm_gaussian_componentwise_bound_network_shapes(case):
    """the same bound at the six network shapes of test_gpu_parity.py::test_train_gemm_and_wgrad_vs_torch_fp64.  Measured worst
    error / bound: 0.21 (K = 24)."""
    M, K, N = case
    g = _gen(K * 7 + N)
    _gemm_gaussian(_te(), M, K, N, dev(torch.randn(N, K, generator=g) / K ** 0.5), dev(torch.randn(K, N, generator=g) / K ** 0.5), None)


# ---------------------------------------------------------------------------------------------------------------------------
# squeeze-excite, fc_small, rows_*_bn at their limits
# ---------------------------------------------------------------------------------------------------------------------------
FWD_TOL, GRAD_TOL = 2e-6, 5e-6         # test_gpu_parity.py::test_se_train_kernels_vs_torch_fp64's bounds
# Cse = 1 and 128 (the admitted maximum), C < 16 (fc1's tail step alone), B = 1, B = 16 / 17 / 15 / 33 around the 16-sample MFMA tile
SE_CASES = [(1, 4, 1), (1, 12, 3), (16, 16, 4), (17, 68, 17), (15, 2304, 128), (33, 40, 127)]
# J = 1, J = 16, B J = 12288 (the admitted maximum), C one quad past a 256-thread block of fc_small_bwd_w
FC_CASES = [(1, 4, 1), (3, 1536, 16), (768, 8, 16), (64, 260, 9)]
ROWS_BN_CASES = [(1, 1, 4), (3, 129, 68), (2, 300, 2304)]


def _se_operands(B, C, Cse, integer):
    g = _gen(B * 1000 + C + Cse + (500000 if integer else 0))
    if integer:
        return ints(g, B, C), ints(g, Cse, C, 1, 1), ints(g, Cse), ints(g, C, Cse, 1, 1), ints(g, C), ints(g, B, C)
    rn = lambda *s: torch.randn(*s, generator=g)
    return rn(B, C), rn(Cse, C, 1, 1) / C ** 0.5, rn(Cse), rn(C, Cse, 1, 1) / Cse ** 0.5, rn(C), rn(B, C)


@pytest.mark.parametrize('B,C,Cse', SE_CASES)
def test_se_forward_h_pre_exact_integers(B, C, Cse):
    """h_pre of cosy_se_train_forward (se_train_fc1: eight waves split C, tail step, LDS combine) on integer pooled / w_reduce / b_reduce:
    W1 pooled + b1 bit for bit."""
    te = _te()
    pooled, w1, b1, w2, b2, _ = _se_operands(B, C, Cse, True)
    assert_exact_range(pooled, w1, C, b1)
    h_pre, _ = te.se_forward(dev(pooled), dev(w1), dev(b1), dev(w2), dev(b2))
    assert torch.equal(h_pre.cpu(), (pooled.double() @ w1.double().view(Cse, C).t() + b1.double()).float())


def _se_run(te, pooled, w1, b1, w2, b2, dgate):
    p, a, b, c, d, dg = (dev(t) for t in (pooled, w1, b1, w2, b2, dgate))
    h_pre, gate = te.se_forward(p, a, b, c, d)
    back = te.se_backward(dg, gate, h_pre, p, a, c)
    again = te.se_backward(dg, gate, h_pre, p, a, c)
    assert all(torch.equal(x, y) for x, y in zip(back, again))           # every sum in a fixed order
    return h_pre, gate, back


@pytest.mark.parametrize('B,C,Cse', SE_CASES)
def test_se_limits_vs_fp64(B, C, Cse):
    """cosy_se_train_forward / _backward at Cse = 1 / 128, C < 16, B = 1 and batches around the 16-sample tile, against float64
    autograd of sigmoid(W2 swish(W1 pooled + b1) + b2): h_pre and gate within 2e-6, the five gradients within 5e-6 (max error over
    max magnitude per tensor); the backward repeated once, bit for bit.  Measured worst: h_pre 2.8e-7, gate 3.3e-7; dpooled 3.1e-7,
    dw_reduce 3.1e-7, db_reduce 3.7e-7, dw_expand 2.1e-7, db_expand 1.9e-7."""
    te = _te()
    pooled, w1, b1, w2, b2, dgate = _se_operands(B, C, Cse, False)
    h_pre, gate, (dpooled, dw1, db1, dw2, db2) = _se_run(te, pooled, w1, b1, w2, b2, dgate)
    P = [t.double().requires_grad_(True) for t in (pooled, w1, b1, w2, b2)]
    hp = P[0] @ P[1].view(Cse, C).t() + P[2]
    gt = torch.sigmoid((hp * torch.sigmoid(hp)) @ P[3].view(C, Cse).t() + P[4])
    gt.backward(dgate.double())
    tag = f'B={B} C={C} Cse={Cse}'
    report(tag + ' h_pre', rel(h_pre, hp.detach()), FWD_TOL)
    report(tag + ' gate', rel(gate, gt.detach()), FWD_TOL)
    for name, got, want in (('dpooled', dpooled, P[0].grad), ('dw_reduce', dw1.view_as(w1), P[1].grad), ('db_reduce', db1, P[2].grad),
                            ('dw_expand', dw2.view_as(w2), P[3].grad), ('db_expand', db2, P[4].grad)):
        report(f'{tag} {name}', rel(got, want), GRAD_TOL)


def test_se_sample_alone_equals_sample_16_of_17():
    """The columns of the 16-sample MFMA tile are independent (header of the kernels): a sample's h_pre, gate and dpooled are the same
    bit for bit alone (B = 1) and as the last sample of a batch of 17 (the second tile's only column)."""
    te = _te()
    pooled, w1, b1, w2, b2, dgate = _se_operands(17, 68, 17, False)
    h17, g17, back17 = _se_run(te, pooled, w1, b1, w2, b2, dgate)
    h1, g1, back1 = _se_run(te, pooled[16:], w1, b1, w2, b2, dgate[16:])
    assert torch.equal(h1, h17[16:]) and torch.equal(g1, g17[16:]) and torch.equal(back1[0], back17[0][16:])


@pytest.mark.parametrize('B,C,J', FC_CASES)
def test_fc_small_exact_integers(B, C, J):
    """cosy_fc_small_forward with an integer bias and cosy_fc_small_backward (dx, dw, db) on integer operands: bit for bit."""
    te = _te()
    g = _gen(B * 1000 + C + J)
    x, w, bias, dy = ints(g, B, C), ints(g, J, C), ints(g, J), ints(g, B, J)
    assert_exact_range(x, w, C, bias)
    assert_exact_range(dy, w, J)
    assert_exact_range(dy, x, B)
    xd, wd, dyd = dev(x), dev(w), dev(dy)
    assert torch.equal(te.fc_small_forward(xd, wd, dev(bias)).cpu(), (x.double() @ w.double().t() + bias.double()).float())
    dx, dw, db = te.fc_small_backward(dyd, xd, wd)
    assert torch.equal(dx.cpu(), (dy.double() @ w.double()).float())
    assert torch.equal(dw.cpu(), (dy.double().t() @ x.double()).float())
    assert torch.equal(db.cpu(), dy.double().sum(0).float())


@pytest.mark.parametrize('B,C,J', FC_CASES)
def test_fc_small_limits_vs_fp64(B, C, J):
    """cosy_fc_small_forward / _backward at J = 1, J = 16, B J = 12288 and C = 260 against float64: y and dx within 2e-6, dw and db
    within 5e-6; the backward repeated once, bit for bit.  Measured worst: y 1.0e-7, dx 1.1e-7, dw 6.6e-7, db 6.0e-7."""
    te = _te()
    g = _gen(B * 1000 + C + J + 1)
    rn = lambda *s: torch.randn(*s, generator=g)
    x, w, bias, dy = rn(B, C), rn(J, C) / C ** 0.5, rn(J), rn(B, J)
    xd, wd, dyd = dev(x), dev(w), dev(dy)
    tag = f'B={B} C={C} J={J}'
    report(tag + ' y', rel(te.fc_small_forward(xd, wd, dev(bias)), x.double() @ w.double().t() + bias.double()), FWD_TOL)
    dx, dw, db = te.fc_small_backward(dyd, xd, wd)
    report(tag + ' dx', rel(dx, dy.double() @ w.double()), FWD_TOL)
    report(tag + ' dw', rel(dw, dy.double().t() @ x.double()), GRAD_TOL)
    report(tag + ' db', rel(db, dy.double().sum(0)), GRAD_TOL)
    assert all(torch.equal(a, b) for a, b in zip(te.fc_small_backward(dyd, xd, wd), (dx, dw, db)))


@pytest.mark.parametrize('B,HW,C', ROWS_BN_CASES)
def test_rows_bn_reductions_vs_fp64(B, HW, C):
    """cosy_rows_mean_bn / cosy_rows_dot_bn (the per-sample mean of swish(bn(raw)) and sum of a * swish(bn(raw)), the activation
    recomputed per element) from one pixel and one channel quad to 2304 channels, against float64 within 5e-6; repeated once, bit for
    bit.  Measured worst: mean 6.1e-8, dot 9.5e-8."""
    te = _te()
    g = _gen(B * 1000 + HW + C)
    rn = lambda *s: torch.randn(*s, generator=g)
    raw, a = rn(B * HW, C), rn(B * HW, C)
    mean, rstd, gamma_, beta = rn(C) * 0.1, rn(C).abs() + 0.5, rn(C), rn(C) * 0.1
    y = (raw.double() - mean.double()) * rstd.double() * gamma_.double() + beta.double()
    a1 = y * torch.sigmoid(y)
    args = [dev(t) for t in (raw, mean, rstd, gamma_, beta)]
    ad = dev(a)
    tag = f'B={B} HW={HW} C={C}'
    m = te.rows_mean_bn(*args, B, HW, C)
    d = te.rows_dot_bn(ad, *args, B, HW, C)
    report(tag + ' rows_mean_bn', rel(m, a1.view(B, HW, C).mean(1)), GRAD_TOL)
    report(tag + ' rows_dot_bn', rel(d, (a.double() * a1).view(B, HW, C).sum(1)), GRAD_TOL)
    assert torch.equal(te.rows_mean_bn(*args, B, HW, C), m) and torch.equal(te.rows_dot_bn(ad, *args, B, HW, C), d)


# ---------------------------------------------------------------------------------------------------------------------------
# argument contract
# ---------------------------------------------------------------------------------------------------------------------------
def test_argument_contract_matrix_kernels():
    """Refusals, all decided on the host before anything is launched: COSY_EINVAL, cosy_last_error() names the entry and the
    offending value, outputs (and, for the GEMM, the workspace its pack kernel would write) keep their sentinel.
    cosy_train_gemm / _gemm_packed / _pack_plan: K or N not a multiple of 8 (the rule of the tile kernel behind them; the message
    says 8), M = 0, null pointers.  cosy_wgrad: M = 0, null pointers.  Squeeze-excite: C = 6, Cse = 129.  fc_small: J = 17,
    B J = 12289.  Every buffer is large enough for the refused shape."""
    te = _te()
    lib, ptr, stream = _abi()
    SENT = 1234.5
    ws = te._workspace('cuda')
    ws_head = ws[:1 << 16].view(torch.float32)

    def expect_einval(rc, names, *outs):
        msg = lib.cosy_last_error().decode()
        assert rc == COSY_EINVAL, (rc, msg)
        for s in names:
            assert s in msg, (s, msg)
        torch.cuda.synchronize()
        for o in outs:
            assert (o == SENT).all(), msg

    buf = lambda n: torch.full((n,), SENT, device='cuda')
    rnd = lambda n: torch.randn(n, device='cuda')
    # ---- GEMM
    A, W, add, out = rnd(4096), rnd(4096), rnd(4096), buf(4096)
    pool = torch.zeros(2 * 4096 + 16 + 4096, device='cuda')
    off = 2 * 4096 + 16                                        # where a first packed weight starts
    gemm = lambda M, K, N, a=A, w=W, o=out, wsp=ws: lib.cosy_train_gemm(ptr(a), ptr(w), 0, M, K, N, ptr(add), ptr(o), ptr(wsp), stream())
    packed = lambda M, K, N, a=A, p=pool, o=out: lib.cosy_train_gemm_packed(ptr(a), ptr(p), off, M, K, N, ptr(add), ptr(o), stream())
    for M, K, N, names in ((16, 12, 16, ['K=12', 'multiples of 8']), (16, 16, 12, ['N=12', 'multiples of 8']), (16, 20, 36, ['K=20', 'N=36', 'of 8']),
                           (0, 16, 16, ['M=0'])):
        ws_head.fill_(SENT)
        expect_einval(gemm(M, K, N), ['train_gemm:'] + names, out, ws_head)
        expect_einval(packed(M, K, N), ['train_gemm_packed:'] + names, out)
    ws_head.fill_(SENT)
    expect_einval(gemm(16, 16, 16, a=None), ['train_gemm:'], out, ws_head)
    expect_einval(gemm(16, 16, 16, w=None), ['train_gemm:'], out, ws_head)
    expect_einval(gemm(16, 16, 16, o=None), ['train_gemm:'], ws_head)
    expect_einval(gemm(16, 16, 16, wsp=None), ['train_gemm:'], out)
    expect_einval(packed(16, 16, 16, a=None), ['train_gemm_packed:'], out)
    expect_einval(packed(16, 16, 16, p=None), ['train_gemm_packed:'], out)
    expect_einval(packed(16, 16, 16, o=None), ['train_gemm_packed:'])
    assert (pool == 0).all()
    # ---- the pack plan (host only)
    plan = torch.full((2, 8), -7, dtype=torch.int64)
    floats, blocks = ctypes.c_longlong(-7), ctypes.c_longlong(-7)

    def plan_rc(Ks, Ns, Wp=None):
        n = len(Ks)
        Wa = (ctypes.c_void_p * n)(*(Wp or [W.data_ptr()] * n))
        return lib.cosy_train_pack_plan(n, Wa, (ctypes.c_int * n)(*Ks), (ctypes.c_int * n)(*Ns), (ctypes.c_int * n)(*[0] * n), plan.data_ptr(),
                                        ctypes.byref(floats), ctypes.byref(blocks))
    for Ks, Ns, names in (([12], [16], ['entry 0', 'K=12', 'multiples of 8']), ([16, 16], [16, 12], ['entry 1', 'N=12', 'multiples of 8']),
                          ([0], [16], ['entry 0', 'K=0'])):
        expect_einval(plan_rc(Ks, Ns), ['train_pack_plan:'] + names)
        assert floats.value == -7 and blocks.value == -7
    expect_einval(plan_rc([16], [16], Wp=[None]), ['train_pack_plan:', 'entry 0'])
    expect_einval(lib.cosy_train_pack_plan(1, None, None, None, None, plan.data_ptr(), ctypes.byref(floats), ctypes.byref(blocks)), ['train_pack_plan:'])
    assert plan_rc([16], [16]) == COSY_OK and floats.value > off       # the same call with a legal shape is accepted
    # ---- wgrad
    dY, X, dW = rnd(4096), rnd(4096), buf(4096)
    expect_einval(lib.cosy_wgrad(ptr(dY), ptr(X), 0, 16, 16, ptr(dW), ptr(ws), stream()), ['wgrad:', 'M=0'], dW)
    expect_einval(lib.cosy_wgrad(None, ptr(X), 16, 16, 16, ptr(dW), ptr(ws), stream()), ['wgrad:'], dW)
    expect_einval(lib.cosy_wgrad(ptr(dY), None, 16, 16, 16, ptr(dW), ptr(ws), stream()), ['wgrad:'], dW)
    expect_einval(lib.cosy_wgrad(ptr(dY), ptr(X), 16, 16, 16, None, ptr(ws), stream()), ['wgrad:'])
    expect_einval(lib.cosy_wgrad(ptr(dY), ptr(X), 16, 16, 16, ptr(dW), None, stream()), ['wgrad:'], dW)
    # ---- squeeze-excite: C = 6 (B = 1, Cse = 4), Cse = 129 (B = 1, C = 8)
    for C, Cse, names in ((6, 4, ['C=6']), (8, 129, ['Cse=129'])):
        ins = [rnd(4096) for _ in range(6)]
        h_pre, gate = buf(4096), buf(4096)
        expect_einval(lib.cosy_se_train_forward(*(ptr(t) for t in ins[:5]), 1, C, Cse, ptr(h_pre), ptr(gate), stream()),
                      ['se_train_forward:'] + names, h_pre, gate)
        outs = [buf(4096) for _ in range(5)]
        expect_einval(lib.cosy_se_train_backward(*(ptr(t) for t in ins), 1, C, Cse, *(ptr(t) for t in outs), ptr(ws), stream()),
                      ['se_train_backward:'] + names, *outs)
    # ---- fc_small: J = 17 (B = 1, C = 8), B J = 12289 (B = 12289, J = 1, C = 4)
    x, w, bias, dy = rnd(12289 * 4), rnd(4096), rnd(4096), rnd(12289)
    y, dx, dw, db = buf(4096), buf(12289 * 4), buf(4096), buf(4096)
    expect_einval(lib.cosy_fc_small_forward(ptr(x), ptr(w), ptr(bias), 1, 8, 17, ptr(y), stream()), ['fc_small_forward:', 'J=17'], y)
    expect_einval(lib.cosy_fc_small_backward(ptr(dy), ptr(x), ptr(w), 1, 8, 17, ptr(dx), ptr(dw), ptr(db), stream()),
                  ['fc_small_backward:', 'J=17'], dx, dw, db)
    expect_einval(lib.cosy_fc_small_backward(ptr(dy), ptr(x), ptr(w), 12289, 4, 1, ptr(dx), ptr(dw), ptr(db), stream()),
                  ['fc_small_backward:', 'B=12289'], dx, dw, db)
    torch.cuda.synchronize()
