"""The backward of the multi-scale RoIAlign into the feature maps on the GPU (cosy_msroi_align_backward in csrc/kernels_detpre.hip behind
cosypose_amd/detector_rpn.py) against the CPU twin tests/detbwd_ref.py, which test_roi_backward_host.py holds against torch's autograd and
hand-computed weights.

Gradients are compared BIT for bit with the float32 twin (the same correctly rounded operations in the same order, contraction off) and
against the float64 twin within  u (n + 4) sum |term|,  u = 2^-24, n the number of terms of the cell (section 24 derives it: a weight
product carries 3 roundings, the product with grad_out 1, the n - 1 additions and the division n).  Every test prints its share of the bound
before it asserts."""
import ctypes

import numpy as np
import pytest
import torch

import detbwd_ref as ref
import detpre_ref as pre
from cosypose_amd import _lib, detector_rpn, detector_train as dt, multiscale_roi_align, roi_align

pytestmark = pytest.mark.gpu
f32 = np.float32
U = 2.0 ** -24
CASES = ref.make_cases()
BY_NAME = {c['name']: c for c in CASES}
SENTINEL, GUARD = -777.0, 64
K_MIN, K_MAX = 2, 6
_TWIN = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def twin(case):
    """float32 twin, float64 twin, sum |term|, number of terms: computed once per case and shared"""
    if case['name'] not in _TWIN:
        args = (case['grad_out'], case['boxes'], case['im_ids'], ref.SHAPES, ref.SCALES, case['P'], case['g'], ref.B)
        _TWIN[case['name']] = (ref.roi_align_backward(*args),) + ref.roi_align_backward(*args, dtype=np.float64)
    return _TWIN[case['name']]


def level_table(shapes=ref.SHAPES, scales=ref.SCALES):
    lv = _lib.MsroiLevels()
    for l, ((H, W), s) in enumerate(zip(shapes, scales)):
        lv.H[l], lv.W[l], lv.scale[l] = H, W, s
    return lv


def backward_direct(case, skip=(), grad_out=None):
    """the C entry point on ONE sentinel-filled buffer that holds guard | level 0 | guard | level 1 | ... | guard -> per level (B,C,H,W), None
    for a level in `skip` (null pointer: untouched); every other cell written, no guard element touched"""
    C, P, g, R = case['C'], case['P'], case['g'], len(case['boxes'])
    sizes = [ref.B * C * H * W for H, W in ref.SHAPES]
    starts = [GUARD + sum(sizes[:l]) + GUARD * l for l in range(len(sizes))]
    buf = torch.full((starts[-1] + sizes[-1] + GUARD,), SENTINEL, dtype=torch.float32, device='cuda')
    ptrs = (ctypes.c_void_p * 8)(*[None if l in skip else buf.data_ptr() + 4 * s for l, s in enumerate(starts)])
    go, boxes = dev(case['grad_out'] if grad_out is None else grad_out), dev(case['boxes'])
    padded = 'rows' in case
    im_id = None if padded else dev(case['im_ids'].astype(np.int32))
    counts = dev(np.array(case['counts'], np.int32)) if padded else None
    ws = torch.full((8 * R + GUARD,), -9, dtype=torch.int32, device='cuda')
    lv = level_table()
    rc = _lib.lib().cosy_msroi_align_backward(ctypes.byref(lv), ptrs, len(sizes), ref.B, C, _lib.ptr(go), _lib.ptr(boxes), _lib.ptr(im_id), _lib.ptr(counts),
                                              case['rows'] if padded else 0, R, P, g, K_MIN, K_MAX, _lib.ptr(ws), None)
    assert rc == 0, _lib.lib().cosy_last_error()
    torch.cuda.synchronize()
    buf, out, at = buf.cpu().numpy(), [], 0
    assert (ws[8 * R:].cpu().numpy() == -9).all()
    for l, (s, n) in enumerate(zip(starts, sizes)):
        assert (buf[at:s] == SENTINEL).all(), f'guard in front of level {l}'
        body, at = buf[s:s + n], s + n
        if l in skip:
            assert (body == SENTINEL).all()
            out.append(None)
        else:
            assert (body != SENTINEL).all()                                      # every cell written
            out.append(body.reshape(ref.B, C, *ref.SHAPES[l]).copy())
    assert (buf[at:] == SENTINEL).all()
    return out


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.int32)


def held(name, got, v64, mag, cnt, extra=0.0):
    """|got - float64 twin| <= u (n + 4) sum |term| (+ extra), level by level; prints the largest share"""
    worst = 0.0
    for g, v, m, n in zip(got, v64, mag, cnt):
        if g is None:
            continue
        bound = U * (n[:, None] + 4) * m + extra * np.abs(v)
        err = np.abs(g.astype(np.float64) - v)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert np.isfinite(g).all() and (err <= bound).all(), name
    print(f'{name}: largest error / bound = {worst:.3f} (bound: 1), most terms on a cell {max(int(n.max()) for n in cnt)}')


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_backward_equals_the_twin(case):
    assert ref.away_from_level_boundaries(case['boxes'])                        # at least 1e-3 from a level boundary
    want, v64, mag, cnt = twin(case)
    got = backward_direct(case)
    for l, (g, w) in enumerate(zip(got, want)):
        assert np.isfinite(g).all() and np.array_equal(bits(g), bits(w)), f'level {l}'          # bit for bit; finite with inf and NaN boxes
        assert not g[np.broadcast_to(cnt[l][:, None] == 0, g.shape)].view(np.int32).any()      # +0 where no term arrives
    held(case['name'], got, v64, mag, cnt)
    again = backward_direct(case)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got, again))                   # two calls, equal bits
    if case['name'] == 'only level 0':
        assert got[0].any() and all(not g.view(np.int32).any() for g in got[1:])              # a level no row maps to: exact zeros
    if case['name'].startswith('grid') and case['P'] >= 7:                      # every level, and cells on both sides of every tile seam
        assert all(n.any() for n in cnt) and all(cnt[0][:, k, :].any() and cnt[0][:, :, k].any() for k in (15, 16, 31, 32))
    if case['name'] == '300 identical rows':
        assert int(cnt[0].max()) >= 300 * 4                                     # more than one list chunk (256 rows) on one cell
    if case['name'] == 'grad_out zero':
        assert all(not g.view(np.int32).any() for g in got)


def test_a_level_that_needs_no_gradient_is_skipped():
    case = BY_NAME['grid C=3 P=7 g=2']
    full = backward_direct(case)
    for skip in ((1,), (0, 4), (0, 1, 2, 3, 4)):
        part = backward_direct(case, skip=skip)
        assert all(p is None if l in skip else np.array_equal(bits(p), bits(full[l])) for l, p in enumerate(part))


def test_adjoint_identity():
    """<multiscale_roi_align(F), G> = <F, backward(G)>, both sides from the device, summed in float64 on the host: equal within the sum of the
    two sides' bounds (section 22's u (g^2 + 8)(1 + 2^-10) sum |w p| per forward value, section 24's per gradient)"""
    case = BY_NAME['grid C=3 P=7 g=2']
    C, P, g = case['C'], case['P'], case['g']
    rng = np.random.RandomState(3)
    feats = [rng.uniform(-2, 2, (ref.B, C, H, W)).astype(f32) for H, W in ref.SHAPES]
    G = case['grad_out'].astype(np.float64)
    out = multiscale_roi_align([dev(t) for t in feats], dev(case['boxes']), None, P, g, batch_im_id=dev(case['im_ids']), scales=ref.SCALES)
    out = out.cpu().numpy().astype(np.float64)
    _, _, fwd_mag = pre.multiscale_roi_align(feats, case['boxes'], case['im_ids'], ref.SCALES, P, g, np.float64)
    grads = backward_direct(case)
    _, _, mag, cnt = twin(case)
    lhs, rhs = float((out * G).sum()), float(sum((f.astype(np.float64) * gr).sum() for f, gr in zip(feats, grads)))
    bound = float((U * (g * g + 8) * (1 + 2.0 ** -10) * fwd_mag * np.abs(G)).sum())
    bound += float(sum((U * (n[:, None] + 4) * m * np.abs(f)).sum() for f, m, n in zip(feats, mag, cnt)))
    print(f'adjoint identity: {lhs!r} vs {rhs!r}, difference / bound = {abs(lhs - rhs) / bound:.3f} (bound: 1)')
    assert abs(lhs) > 1 and abs(lhs - rhs) <= bound


# ---- autograd ------------------------------------------------------------------------------------------------------------------------
def test_autograd_through_multiscale_roi_align():
    case = BY_NAME['grid C=3 P=7 g=2']
    C, P, g = case['C'], case['P'], case['g']
    rng = np.random.RandomState(4)
    host = [rng.uniform(-2, 2, (ref.B, C, H, W)).astype(f32) for H, W in ref.SHAPES]
    boxes, ids, G = dev(case['boxes']), dev(case['im_ids']), dev(case['grad_out'])
    run = lambda feats: multiscale_roi_align(feats, boxes, None, P, g, batch_im_id=ids, scales=ref.SCALES)
    plain = run([dev(t) for t in host])
    assert not plain.requires_grad and plain.grad_fn is None                    # no feature requires grad: the old path
    feats = [dev(t).requires_grad_(True) for t in host]
    with torch.no_grad():
        quiet = run(feats)
    assert not quiet.requires_grad and quiet.grad_fn is None and torch.equal(quiet, plain)
    out = run(feats)
    assert out.requires_grad and torch.equal(out, plain)                        # the forward bits are the same launch's
    grads = torch.autograd.grad((out * G).sum() * 2.5, feats)                   # grad_out = fl(2.5 G)
    want = backward_direct(case, grad_out=case['grad_out'] * f32(2.5))
    assert all(np.array_equal(bits(a.cpu().numpy()), bits(w)) for a, w in zip(grads, want))
    # a grad_out that is not contiguous: (R,P,P,C) storage seen as (R,C,P,P)
    odd = dev(np.ascontiguousarray(case['grad_out'].transpose(0, 2, 3, 1))).permute(0, 3, 1, 2)
    assert not odd.is_contiguous()
    same = torch.autograd.grad(run(feats), feats, grad_outputs=odd)
    assert all(np.array_equal(bits(a.cpu().numpy()), bits(w)) for a, w in zip(same, backward_direct(case)))
    # one level that does not require grad: None for it, the others unchanged
    mixed = [f.detach().requires_grad_(l != 1) for l, f in enumerate(feats)]
    (run(mixed) * G).sum().backward()
    assert mixed[1].grad is None
    assert all(np.array_equal(bits(m.grad.cpu().numpy()), bits(w)) for l, (m, w) in enumerate(zip(mixed, backward_direct(case))) if l != 1)
    # return_levels rides along without a gradient
    out, levels = multiscale_roi_align(feats, boxes, None, P, g, batch_im_id=ids, scales=ref.SCALES, return_levels=True)
    assert out.requires_grad and not levels.requires_grad and levels.dtype == torch.int32


def test_autograd_through_roi_align():
    H, W = ref.SHAPES[0]
    boxes = ref.all_boxes()[:9]                                                 # the seam boxes and the wide one
    ids = (np.arange(len(boxes)) % ref.B).astype(np.int64)
    rng = np.random.RandomState(6)
    x = dev(rng.uniform(-2, 2, (ref.B, 3, H, W)).astype(f32)).requires_grad_(True)
    G = rng.uniform(-2, 2, (len(boxes), 3, 7, 7)).astype(f32)
    rois = dev(np.concatenate([ids[:, None].astype(f32), boxes], 1))
    out = roi_align(x, rois, 7, 0.25, 2)
    multi = multiscale_roi_align([x.detach()], dev(boxes), None, 7, 2, batch_im_id=dev(ids), scales=[0.25])
    assert torch.equal(out, multi)
    grad, = torch.autograd.grad(out, x, grad_outputs=dev(G) * 0.5)
    want = ref.roi_align_backward(G * f32(0.5), boxes, ids, [(H, W)], [0.25], 7, 2, ref.B)[0]
    assert np.array_equal(bits(grad.cpu().numpy()), bits(want)) and want.any()
    by_image = [dev(boxes[ids == b]) for b in range(ref.B)]                     # the list form: image by image
    listed = roi_align(x, by_image, 7, 0.25, 2)
    assert torch.equal(listed, torch.cat([out[dev(ids) == b] for b in range(ref.B)]))
    empty = roi_align(x, rois[:0], 7, 0.25)                                      # no row: zeros for every cell
    grad, = torch.autograd.grad(empty.sum(), x)
    assert tuple(empty.shape) == (0, 3, 7, 7) and not grad.any()


# ---- the chain -----------------------------------------------------------------------------------------------------------------------
GRID, A = [(5, 7), (3, 4), (1, 2)], 3                                          # section 23's grid
SIZES, RATIOS = ((32,), (64,), (128,)), (0.5, 1.0, 2.0)
PAD, NETS = (40, 56), [(37, 53), (40, 50)]
N_ANCHORS = sum(A * H * W for H, W in GRID)
CHAIN_RPN = dict(pre_nms_top_n=64, post_nms_top_n=20)


class Heads:
    """test_detector_train.py's tiny heads: the RPN's size deltas are zero; the box and mask heads run in float64 and round once"""

    def __init__(self, seed=0, C=8, K=3):
        g = torch.Generator().manual_seed(seed)
        self.conv, self.logit, self.delta = torch.nn.Conv2d(C, C, 3, padding=1), torch.nn.Conv2d(C, A, 1), torch.nn.Conv2d(C, 4 * A, 1)
        self.fc, self.cls, self.reg = torch.nn.Linear(C * 49, 16).double(), torch.nn.Linear(16, K).double(), torch.nn.Linear(16, 4 * K).double()
        self.mask = torch.nn.Linear(C, K).double()
        self.modules = (self.conv, self.logit, self.delta, self.fc, self.cls, self.reg, self.mask)
        with torch.no_grad():
            for m in self.modules:
                for p in m.parameters():
                    p.copy_((torch.randn(p.shape, generator=g) * (0.3 if p.dim() > 1 else 0.1)).to(p.dtype))
            self.delta.weight.view(A, 4, C)[:, 2:] = 0
            self.delta.bias.view(A, 4)[:, 2:] = 0
            self.reg.weight *= 0.2
        for m in self.modules:
            m.cuda()

    def rpn(self, feats):
        hidden = [torch.relu(self.conv(f)) for f in feats]
        return [self.logit(h) for h in hidden], [self.delta(h) for h in hidden]

    def box(self, roi):
        h = torch.relu(self.fc(roi.flatten(1).double()))
        return self.cls(h).float(), self.reg(h).float()

    def mask_head(self, roi):
        return self.mask(roi.double().permute(0, 2, 3, 1)).permute(0, 3, 1, 2).float().contiguous()


def test_detector_losses_reach_the_trunk(monkeypatch):
    rng = np.random.RandomState(21)
    gt = [np.array([[8, 0, 40, 32], [20, 10, 50, 36], [0, 0, 20, 18]], f32), np.array([[2, 3, 30, 30], [25, 5, 50, 35]], f32)]
    labels = [[1, 2, 1], [2, 1]]
    masks = [(rng.uniform(0, 1, (len(g), 40, 56)) < 0.5).astype(np.uint8) for g in gt]
    keys = dict(rpn=rng.randint(0, 2 ** 31 - 1, (2, N_ANCHORS)).astype(np.int32), roi=rng.randint(0, 2 ** 31 - 1, (2, 20 + 3)).astype(np.int32))
    targets = [dict(boxes=dev(g), labels=dev(np.asarray(l, np.int64)), masks=dev(m)) for g, l, m in zip(gt, labels, masks)]
    torch.manual_seed(5)
    trunk = torch.nn.Conv2d(3, 8, 3, padding=1).cuda()                          # a small trunk: images of each level's size -> the feature maps
    images = [dev(rng.normal(0, 1, (2, 3, H, W)).astype(f32)) for H, W in GRID]
    features = [trunk(im) for im in images]
    for f in features:
        f.retain_grad()
    seen = []
    launch = detector_rpn.multiscale_roi_align

    def recorded(maps, boxes, net_sizes, output_size, sampling_ratio=2, **kw):
        out = launch(maps, boxes, net_sizes, output_size, sampling_ratio, **kw)
        out.retain_grad()
        seen.append(dict(out=out, boxes=boxes.cpu().numpy(), counts=kw['counts'].cpu().numpy(), P=output_size, g=sampling_ratio))
        return out
    monkeypatch.setattr(detector_rpn, 'multiscale_roi_align', recorded)
    heads = Heads()
    losses = dt.detector_losses(features, heads.rpn, heads.box, heads.mask_head, targets, NETS, PAD, n_roi_levels=2,
                                keys={k: dev(v) for k, v in keys.items()}, sizes=SIZES, aspect_ratios=RATIOS, **CHAIN_RPN)
    assert [s['P'] for s in seen] == [7, 14] and all(s['out'].requires_grad for s in seen)
    (losses['loss_classifier'] + losses['loss_box_reg'] + losses['loss_mask']).backward(retain_graph=True)
    assert features[0].grad is not None and features[1].grad is not None        # (fails before this feature: the RoI maps were detached)
    assert features[2].grad is None                                             # not a RoI level, and no RPN loss yet
    shapes, scales = GRID[:2], pre.infer_scales(GRID[:2], NETS)
    parts32, parts64 = [], []
    for s in seen:
        go, rows = s['out'].grad.cpu().numpy(), len(s['boxes']) // 2
        assert go.any() and int(s['counts'].min()) >= 1
        args = (go, s['boxes'], ref.padded_im_ids(2, rows, s['counts']), shapes, scales, s['P'], s['g'], 2)
        parts32.append(ref.roi_align_backward(*args))
        parts64.append(ref.roi_align_backward(*args, dtype=np.float64))
    for l in range(2):
        got = features[l].grad.cpu().numpy()
        assert np.array_equal(bits(got), bits(parts32[0][l] + parts32[1][l]))   # the twin's bits, added once by autograd
        # no box of a 40 x 56 image reaches the 224 px of level 1: every RoI maps to level 0, and level 1 receives its exact zeros
        assert got.any() == (l == 0) and all(bool(p[2][l].any()) == (l == 0) for p in parts64)
        v = parts64[0][0][l] + parts64[1][0][l]
        bound = sum(U * (p[2][l][:, None] + 4) * p[1][l] for p in parts64) + U * np.abs(v)
        err = np.abs(got.astype(np.float64) - v)
        print(f'chain feature {l}: largest error / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f} (bound: 1)')
        assert (err <= bound).all()
    for name, p in trunk.named_parameters():                                    # the three RoI losses alone already train the trunk
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.any()), name
    before = {n: p.grad.clone() for n, p in trunk.named_parameters()}
    (losses['loss_objectness'] + losses['loss_rpn_box_reg']).backward()         # with the two RPN losses added
    for name, p in trunk.named_parameters():
        assert bool(torch.isfinite(p.grad).all()) and bool(p.grad.any()) and not torch.equal(p.grad, before[name]), name
    assert features[2].grad is not None


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_c_abi_refusals():
    lib, ptr = _lib.lib(), _lib.ptr
    R, C, P = 6, 3, 7
    case = BY_NAME['grid C=3 P=7 g=2']
    boxes, ids = dev(case['boxes'][:R]), dev(case['im_ids'][:R].astype(np.int32))
    counts, go = dev(np.array([3, 2], np.int32)), dev(case['grad_out'][:R])
    grads = [torch.full((ref.B, C, H, W), 7.0, device='cuda') for H, W in ref.SHAPES]
    ws = torch.full((8 * R,), 7, dtype=torch.int32, device='cuda')
    table = lambda only=None: (ctypes.c_void_p * 8)(*[t.data_ptr() if only is None or l in only else None for l, t in enumerate(grads)])

    def levels(**change):
        lv = level_table()
        for field, (l, v) in change.items():
            getattr(lv, field)[l] = v
        return ctypes.byref(lv)
    good = dict(lv=levels(), grads=table(), L=5, B=ref.B, C=C, go=ptr(go), boxes=ptr(boxes), im_id=ptr(ids), counts=None, rows=0, R=R, P=P, g=2,
                k_min=K_MIN, k_max=K_MAX, ws=ptr(ws), s=None)
    call = lambda **change: lib.cosy_msroi_align_backward(*{**good, **change}.values())
    bads = [dict(lv=None), dict(L=0), dict(L=9), dict(B=-1), dict(R=-1), dict(C=0), dict(g=0), dict(g=-2), dict(P=0), dict(P=65), dict(P=7, g=19),
            dict(k_min=7), dict(k_max=7), dict(im_id=None), dict(rows=3), dict(im_id=None, rows=0, counts=ptr(counts)), dict(counts=ptr(counts)),
            dict(B=0), dict(lv=levels(H=(1, 0))), dict(lv=levels(W=(3, -1))), dict(lv=levels(H=(0, 1 << 15), W=(0, 1 << 15))),
            dict(lv=levels(scale=(2, 0.0))), dict(lv=levels(scale=(0, float('nan')))),
            dict(grads=None), dict(R=(1 << 30) + 1), dict(C=32 * 65535 + 1), dict(B=1 << 28),                 # the limits of the backward alone
            dict(go=None), dict(boxes=None), dict(ws=None)]
    for bad in bads:
        assert call(**bad) != 0 and b'cosy_msroi_align_backward' in lib.cosy_last_error(), bad
        torch.cuda.synchronize()
        assert all(bool((t == 7).all()) for t in grads) and bool((ws == 7).all()), bad          # refused before any launch
    # nothing to write: no level asked for, or no image
    assert call(grads=table(only=()), go=None, boxes=None, ws=None) == 0
    assert call(B=0, R=0, im_id=None, rows=1, go=None, boxes=None, ws=None) == 0
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in grads)
    # no row: every cell of every requested level is +0
    assert call(R=0, im_id=None, rows=1, go=None, boxes=None, ws=None, grads=table(only=(0, 3))) == 0
    torch.cuda.synchronize()
    assert all(bool((t == (0 if l in (0, 3) else 7)).all()) for l, t in enumerate(grads))
    assert call(im_id=None, rows=3, counts=ptr(counts)) == 0 and call() == 0
