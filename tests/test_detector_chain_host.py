"""CPU tests that guard tests/detector_chain_ref.py, the plain-torch float64 statement of the detector's training forward that
tests/test_detector_chain.py holds the device to: gradcheck of its RoIAlign, agreement with the twins as a third opinion,
its teeth (nine planted mistakes, each far above the device test's tolerance; the three that only the cases `four-levels` and `mixed` can see move
not one bit on the two earlier cases), what each chosen case reaches, and the cases' stability: the float64 graph and its float32 replica take the
same side at every kink."""
import functools

import numpy as np
import pytest
import torch

import detector_chain_case as cc
import detector_chain_ref as cr
import detpre_ref as pre
import dettrain_ref as tr
import dettrunk_case as tc

F64 = torch.float64
FACTOR = 4                                        # test_detector_chain.py: the device stays within FACTOR x the float32 replica's own error


@functools.lru_cache(maxsize=None)
def step(case, dtype=F64, storage=None, mutate=None):
    """one step of the reference on the twins' CPU inputs -> losses, gradients, map gradients, kinks: computed once and shared"""
    chain = cr.Chain(tc.detector_weights(), dtype=dtype, storage=storage, mutate=mutate)
    return chain.step(cc.cpu_inputs(case)) + (list(chain.kinks),)


def ratios(got, want):
    assert set(got) == set(want)
    return {k: float((got[k].double() - want[k].double()).norm() / want[k].double().norm()) for k in want}


def tolerance(case):
    """what test_detector_chain.py allows a gradient on this case: FACTOR x e32, the float32 replica's largest relative error"""
    return FACTOR * max(ratios(step(case, torch.float32)[1], step(case)[1]).values())


def close(name, got, want, rel=1e-12):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    err = float(np.abs(got - want).max() / max(float(np.abs(want).max()), 1e-300)) if want.size else 0.0
    print(f'{name}: largest |reference - twin| / max |twin| = {err:.2e} (bound: {rel:.0e})')
    assert err <= rel, name


# ---- the RoIAlign ------------------------------------------------------------------------------------------------------------------------
ROI_SHAPES, ROI_SCALES = [(6, 8), (3, 4)], [0.25, 0.125]
# inside, across the right and the bottom border, across the top left corner, wholly outside (twice), smaller than one cell, one per level
ROI_BOXES = [[4.5, 3.25, 20.75, 17.5], [18.0, 10.0, 45.5, 31.0], [-9.0, -6.5, 7.25, 9.0], [60.0, 40.0, 90.0, 70.0], [-50.0, -40.0, -9.5, -8.0],
             [13.3, 9.1, 13.9, 9.6], [2.0, 1.0, 27.0, 22.0], [20.0, 12.0, 52.0, 40.0], [70.0, 50.0, 99.0, 80.0], [9.2, 6.1, 10.4, 7.3]]
ROI_LEVELS, ROI_IMAGES = [0, 0, 0, 0, 0, 0, 1, 1, 1, 1], [0, 1, 0, 1, 0, 1, 1, 0, 1, 0]


def roi_maps(dtype=F64, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn((2, 3, H, W), generator=g, dtype=F64).to(dtype) for H, W in ROI_SHAPES]


@pytest.mark.parametrize('P,g', [(7, 2), (2, 3)])
def test_gradcheck_of_the_roi_align_with_respect_to_the_maps(P, g):
    boxes, im, levels = torch.tensor(ROI_BOXES, dtype=F64), torch.tensor(ROI_IMAGES), torch.tensor(ROI_LEVELS)
    maps = [m.requires_grad_(True) for m in roi_maps()]
    fn = lambda m0, m1: cr.multiscale_roi_align([m0, m1], ROI_SCALES, boxes, im, levels, P, g)
    assert torch.autograd.gradcheck(fn, tuple(maps), eps=1e-6, atol=1e-9, rtol=1e-7)
    out = fn(*maps)
    assert tuple(out.shape) == (len(ROI_BOXES), 3, P, P)
    outside = [3, 4, 8]
    assert not out[outside].any() and out[[0, 1, 2, 5, 6, 7, 9]].abs().flatten(1).max(1).values.min() > 0       # a sample outside [-1, size] is 0
    # the box smaller than a cell is widened to one cell (max(extent, 1)): it touches a 3 x 3 window of map 0 and nothing else, the boxes outside
    # touch nothing, and the weights of an output element that lies inside the map sum to 1
    grads = torch.autograd.grad(out[outside].sum() + out[5].sum(), maps, allow_unused=True)
    window = torch.zeros_like(grads[0], dtype=torch.bool)
    window[1, :, 2:5, 3:6] = True
    assert grads[0][window].all() and not grads[0][~window].any() and abs(float(grads[0].sum()) - 3 * P * P) < 1e-9
    assert grads[1] is None or not grads[1].any()


def test_a_coordinate_at_or_below_zero_is_zero_and_the_last_cell_has_no_upper_neighbour():
    feat = torch.arange(1, 13, dtype=F64).reshape(1, 1, 3, 4)
    # scale 1, P = 1, g = 1: the one sample sits at the box's centre
    centre = lambda x, y: float(cr.roi_align(feat, torch.zeros(1, dtype=torch.long), torch.tensor([[x - 1, y - 1, x + 1, y + 1]], dtype=F64), 1.0, 1, 1, 1))
    assert centre(-0.5, -0.75) == 1.0 and centre(-1.0, 0.0) == 1.0            # clamped to the first cell
    assert centre(-1.01, 1.0) == 0.0 and centre(1.0, 3.01) == 0.0              # outside [-1, size]: nothing
    assert centre(3.5, 2.5) == 12.0 and centre(4.0, 3.0) == 12.0               # past the last cell's centre, up to size: the last cell
    assert centre(1.5, 0.0) == 2.5 and centre(1.0, 1.25) == 7.0                # bilinear in between
    kinks = []
    cr.roi_align(feat, torch.zeros(1, dtype=torch.long), torch.tensor([[0.0, 0.0, 4.0, 3.0]], dtype=F64), 1.0, 2, 1, 1, kinks)
    floors = dict(kinks)
    assert floors['roi_align x floor'].tolist() == [[0.5, 2.5]] and floors['roi_align y floor'].tolist() == [[0.0, 2.0]]    # x: ON a border; y: 0.75 and 2.25


# ---- a third opinion: the twins in float64 -------------------------------------------------------------------------------------------------
def test_the_roi_align_and_the_mask_targets_agree_with_the_twins_in_float64(monkeypatch):
    monkeypatch.setattr(pre, 'F', np.float64)                                  # the twins form the sample positions in their F
    monkeypatch.setattr(tr, 'F', np.float64)
    rng = np.random.RandomState(17)
    corner = rng.uniform(-60, -20, (6, 2))
    large = np.concatenate([corner, corner + rng.uniform(115, 170, (6, 2))], 1)                       # sqrt(area) >= 112: level 1
    boxes = np.concatenate([np.asarray(ROI_BOXES), np.sort(rng.uniform(-20, 80, (12, 2, 2)), 1).reshape(12, 4), large]).astype(np.float32)
    im = np.concatenate([ROI_IMAGES, rng.randint(0, 2, 18)])
    maps = roi_maps(torch.float32)                                              # float32 values, as the device hands them on
    k_min, k_max = 2, 3
    for P, g in ((7, 2), (14, 2), (3, 1)):
        want, levels = pre.multiscale_roi_align([m.numpy() for m in maps], boxes, im, ROI_SCALES, P, g, dtype=np.float64)
        assert want.dtype == np.float64 and set(levels.tolist()) == {0, 1} and np.array_equal(levels, pre.map_levels(boxes, k_min, k_max))
        got = cr.multiscale_roi_align([m.double() for m in maps], ROI_SCALES, torch.from_numpy(boxes).double(), torch.from_numpy(im), torch.from_numpy(levels), P, g)
        close(f'multi-scale RoIAlign P={P} g={g}', got.numpy(), want)
    masks = [(rng.uniform(0, 1, (2, 37, 53)) < 0.6).astype(np.uint8), (rng.uniform(0, 1, (3, 45, 40)) < 0.6).astype(np.uint8)]
    matched = np.array([rng.randint(0, len(masks[b])) for b in im])
    for M in (28, 5):
        want = np.zeros((len(boxes), M, M))
        for b in range(2):
            want[im == b] = tr.mask_targets(masks[b], boxes[im == b], matched[im == b], M)
        kinks = []
        got = cr.mask_targets([torch.from_numpy(m) for m in masks], torch.from_numpy(boxes).double(), torch.from_numpy(im), torch.from_numpy(matched), M, F64, kinks)
        assert int(dict(kinks)['mask target grid'].max()) >= 4 and int(dict(kinks)['mask target grid'].min()) == 1       # adaptive: several grids met
        close(f'mask targets M={M}', got.numpy(), want)


def test_the_encodes_and_the_five_loss_terms_agree_with_the_twins_in_float64():
    rng = np.random.RandomState(23)
    f32 = lambda a: np.asarray(a, np.float32)
    prop = f32(np.sort(rng.uniform(0, 60, (40, 2, 2)), 1).reshape(40, 4) + [0, 0, 1, 1])
    gt_rows = f32(np.sort(rng.uniform(0, 60, (40, 2, 2)), 1).reshape(40, 4) + [0, 0, 1, 1])
    for weights in (cr.RPN_WEIGHTS, cr.ROI_WEIGHTS):
        want = tr.encode(gt_rows, prop, weights, np.float64)[0]
        close(f'encode {weights}', cr.encode(torch.from_numpy(gt_rows).double(), torch.from_numpy(prop).double(), weights).numpy(), want)
    # the RPN's losses on section 23's grid: the twin matches and samples, the reference reads its decisions
    grid, A, pad = [(5, 7), (3, 4), (1, 2)], 3, (40, 56)
    sizes = ((32,), (64,), (128,))
    objectness = [f32(rng.normal(0, 2, (2, A, H, W))) for H, W in grid]
    deltas = [f32(rng.normal(0, 0.5, (2, 4 * A, H, W))) for H, W in grid]
    gt = [f32([[8, 0, 40, 32], [20, 10, 50, 36], [0, 0, 20, 18]]), f32([[2, 3, 30, 30], [25, 5, 50, 35]])]
    N = A * sum(H * W for H, W in grid)
    twin = tr.rpn_loss(objectness, deltas, gt, pad, sizes, cc.RATIOS, rng.randint(0, 2 ** 31 - 1, (2, N)), batch_size_per_image=48)
    assert all(0 < int((m[s] >= 0).sum()) < len(s) for m, s in zip(twin['matched'], twin['sampled']))
    flat = [pre.flatten_level(o[b], d[b]) for b in range(2) for o, d in zip(objectness, deltas)]
    logits = torch.from_numpy(np.stack([np.concatenate([f[0] for f in flat[3 * b:3 * b + 3]]) for b in range(2)])).double()
    rel = torch.from_numpy(np.stack([np.concatenate([f[1] for f in flat[3 * b:3 * b + 3]]) for b in range(2)])).double()
    got = cr.rpn_losses(logits, rel, torch.from_numpy(pre.anchors(grid, pad, sizes, cc.RATIOS)).double(), [torch.from_numpy(g).double() for g in gt],
                        torch.from_numpy(twin['matched']), cc.padded(twin['sampled'], 48, -1, np.int64).reshape(2, 48), torch.tensor([len(s) for s in twin['sampled']]))
    close('loss_objectness', float(got[0]), twin['losses']['loss_objectness'])
    close('loss_rpn_box_reg', float(got[1]), twin['losses']['loss_rpn_box_reg'])
    # Fast R-CNN: 30 real rows, a third of them background; differences on both sides of smooth-L1's beta
    R, K = 30, 3
    z, d = f32(rng.normal(0, 3, (R, K))), f32(rng.normal(0, 1.5, (R, 4 * K)))
    labels, t = rng.randint(0, K, R), f32(rng.normal(0, 1.0, (R, 4)))
    twin = tr.fastrcnn_loss(z, d, labels, t)
    kinks = []
    got = cr.fastrcnn_losses(torch.from_numpy(z).double(), torch.from_numpy(d).double(), torch.from_numpy(labels), torch.from_numpy(t).double(), kinks)
    assert 0 < int(dict(kinks)['smooth l1 branch'].sum()) < dict(kinks)['smooth l1 branch'].numel()
    close('loss_classifier', float(got[0]), twin['losses']['loss_classifier'])
    close('loss_box_reg', float(got[1]), twin['losses']['loss_box_reg'])
    # the mask loss: logits large enough for the stable form of the BCE to matter
    x, lab, tg = f32(rng.normal(0, 20, (5, K, 28, 28))), rng.randint(1, K, 5), f32(rng.uniform(0, 1, (5, 28, 28)))
    want = tr.mask_loss(x, lab, tg, np.ones(5, bool))[0]
    close('loss_mask', float(cr.mask_loss(torch.from_numpy(x).double(), torch.from_numpy(lab), torch.from_numpy(tg).double())), want)


# ---- the trunk as the reference walks it, and the storage points -------------------------------------------------------------------------------
def test_the_layerwise_trunk_is_the_modules_forward_and_the_storage_rounding_goes_straight_through():
    chain = cr.Chain(tc.detector_weights())
    images = cc.cpu_inputs('small')['images'].double()
    with torch.no_grad():
        assert all(torch.equal(a, b) for a, b in zip(chain.trunk_forward(images), chain.trunk(images)))
    assert set(chain.named_parameters()) == {k for k, v in tc.detector_weights().items() if k.endswith(('weight', 'bias')) and not ('.bn' in k or 'downsample.1' in k
                                                                                                                                   or 'body.conv1' in k or 'body.layer1.' in k)}
    x = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -9, -3.0e-5, 0.0], dtype=F64, requires_grad=True)      # a tie to even, above a tie, a small value
    y = cr._Stored.apply(x, True, True)
    assert torch.equal(y.detach(), x.detach().to(torch.bfloat16).double()) and y[0] == 1.0 and y[1] == 1.0 + 2.0 ** -7
    g = torch.tensor([1.0 + 2.0 ** -8, 0.3, -7.0, 1.0 + 3 * 2.0 ** -9], dtype=F64)
    y.backward(g)
    assert torch.equal(x.grad, g.to(torch.bfloat16).double()) and not torch.equal(x.grad, g)
    x.grad = None
    cr._Stored.apply(x, True, False).backward(g)                                   # a packed weight: its gradient stays as it is
    assert torch.equal(x.grad, g)


# ---- teeth: each planted mistake moves a gradient by far more than the device test allows ----------------------------------------------------------
SEEN_ON = dict(level1_reads_map0='two-levels', level2_reads_map1='four-levels', level3_reads_map2='four-levels', gt_rows_at_gmax_stride='mixed')


@pytest.mark.parametrize('mutation', cr.MUTATIONS)
def test_a_planted_mistake_is_seen(mutation):
    case = SEEN_ON.get(mutation, 'small')
    if case in ('four-levels', 'mixed'):                                           # the two earlier cases are blind to it: not one bit moves
        for blind in ('small', 'two-levels'):
            same = step(blind, mutate=mutation)[1], step(blind)[1]
            assert set(same[0]) == set(same[1]) and all(torch.equal(same[0][k], same[1][k]) for k in same[1]), (mutation, blind)
            assert all(torch.equal(a, b) for a, b in zip(step(blind, mutate=mutation)[2], step(blind)[2]))
    tol = tolerance(case)
    moved = ratios(step(case, mutate=mutation)[1], step(case)[1])
    worst = max(moved, key=moved.get)
    print(f'{mutation} on {case}: moves {worst} by {moved[worst]:.3e} = {moved[worst] / tol:.0f} x the tolerance {tol:.3e} (needed: more than 100 x)')
    assert 0 < tol < 1e-4 and moved[worst] > 100 * tol
    if mutation == 'pool_detached':                                                # and it is the pool level's share that went missing
        assert step(case, mutate=mutation)[2][4] is None and step(case)[2][4] is not None and step(case)[2][4].any()
    if mutation == 'rpn_box_over_positives':                                      # only the RPN's regression branch moves
        assert moved['roi_heads.box_head.fc6.weight'] == 0 and moved['rpn.head.cls_logits.bias'] == 0


# ---- the chosen cases ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', list(cc.CASES))
def test_the_float64_graph_and_its_float32_replica_take_the_same_side_at_every_kink(case):
    kinks64, kinks32 = step(case)[3], step(case, torch.float32)[3]
    names = {k.split(' level')[0].split(' image')[0] for k, _ in kinks64}
    assert {'rpn l1 sign', 'smooth l1 branch', 'smooth l1 sign', 'box roi_align', 'mask roi_align', 'mask target grid', 'mask target', 'body.layer2.0.conv1',
            'body.layer4.2', 'rpn.head.cls_logits', 'roi_heads.box_head.fc7', 'roi_heads.mask_predictor.mask_fcn_logits'} <= names
    differ = cr.kink_disagreements(kinks64, kinks32)
    decisions = sum(v.numel() for _, v in kinks64)
    on_a_border = sum(int((v % 1 == 0.5).sum()) for k, v in kinks64 if k.endswith('floor'))
    print(f'{case}: {len(kinks64)} kink tensors, {decisions} decisions, {on_a_border} RoIAlign samples on a cell border, disagreements: {differ}')
    assert not differ


@pytest.mark.parametrize('case', list(cc.CASES))
def test_a_case_reaches_what_it_was_chosen_for(case):
    """on the twins' decisions: one frame with RoIs on all four levels of both paths; three frames of three network sizes with 1, 3 and 5 ground
    truths, among them a tiny one, an all-zero and an all-one mask, each the match of a sampled positive (detector_chain_case.check_reach)"""
    cc.check_reach(case, cc.cpu_inputs(case), step(case)[3])


def test_the_second_case_leaves_level_zero_on_both_paths():
    inp = cc.cpu_inputs('two-levels')
    assert inp['padded_size'] == (160, 224)
    for b, g in enumerate(inp['gt_boxes']):
        assert len(g) == 1 and float(g[0, 2] - g[0, 0]) > 130 and float(g[0, 3] - g[0, 1]) > 130
        n, k = int(inp['roi_counts'][b]), int(inp['pos_counts'][b])
        assert k >= 2 and int((inp['roi_labels'][b * cc.ROI_BATCH:b * cc.ROI_BATCH + n] == 0).sum()) >= 1
    real = lambda key, counts, per: torch.cat([inp[key][b * per:b * per + int(c)] for b, c in enumerate(inp[counts])])
    assert len(set(real('roi_levels', 'roi_counts', cc.ROI_BATCH).tolist())) >= 2 and len(set(real('pos_levels', 'pos_counts', cc.ROI_POSITIVES).tolist())) >= 2
    assert not cc.cpu_inputs('small')['roi_levels'].any()                           # the first case stays on level 0
