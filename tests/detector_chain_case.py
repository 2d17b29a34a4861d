"""The cases that tests/test_detector_chain_host.py (CPU) and tests/test_detector_chain.py (GPU) share: seeded frames, targets and sampler keys
for one training step of the narrow detector of dettrunk_case.detector_weights(), and the inputs of detector_chain_ref.Chain taken from the
twins' chain on the CPU (the GPU test takes them from the device run instead).  The seeds were chosen on the CPU so that the float64 graph and
its float32 replica take the same side at every kink (test_detector_chain_host.py keeps that check), and so that each case reaches what it is
there for (check_reach, run by the CPU test on the twins' decisions and by every GPU test on the device's own)."""
import functools
import math

import numpy as np
import torch

import dethead_case as hc
import detin_ref
import detpre_ref as pre
import dettrain_ref as tr
import dettrunk_case as tc

SIZES, RATIOS = ((32,), (64,), (128,), (256,), (512,)), (0.5, 1.0, 2.0)        # Detector's anchors
RPN_BATCH, ROI_BATCH, ROI_POSITIVES, TOP_N = 256, 512, 128, 2000               # torchvision's training values, as detector_losses has them
N_STAGES = len(tc.BLOCKS)

# name -> frame sizes (h, w), input_resize, seeds of the frames / the masks / the keys, ground truths per frame (x1, y1, x2, y2, label[, mask
# fill]): the share of the box's pixels that its mask holds, MASK_FILL unless given; 0.0 is an all-zero mask, 1.0 the whole box
MASK_FILL = 0.8
CASES = {
    # tests/test_detector_trunk_backward.py's end-to-end frames and targets: 64 x 64 after padding, every RoI on level 0
    'small': dict(frames=tc.E2E_FRAMES, resize=(48, 64), seeds=(31, 41, 5),
                  gt=[[(3, 4, w - 12, h - 9, 1), (w // 3, h // 4, w - 4, h - 3, 2)] for h, w in tc.E2E_FRAMES]),
    # 160 x 224 after the resize, one ground truth per frame whose sides exceed 130 px there: the smallest frames at which the level mapper
    # leaves level 0 (sqrt(area) >= 112)
    'two-levels': dict(frames=[(120, 168), (150, 200)], resize=(160, 224), seeds=(32, 42, 6),
                       gt=[[(0, 0, 118, 103, 1)], [(0, 24, 127, 150, 2)]]),
    # ONE frame that the resize leaves as it is: 448 px is the smallest side at which the level mapper reaches level 3 (sqrt(area) >= 448), so
    # 480 x 640 with a ground truth over nearly the whole frame is the smallest case whose RoIs read and write all four maps.  The other three
    # ground truths sit on levels 1, 0 and 0
    'four-levels': dict(frames=[(480, 640)], resize=(480, 640), seeds=(33, 43, 7),
                        gt=[[(10, 5, 630, 475, 1), (20, 30, 320, 290, 2), (400, 100, 540, 230, 1), (50, 300, 110, 350, 2)]]),
    # three frames (an odd batch) of three shapes, so three network sizes on one 64 x 64 canvas, with 1, 3 and 5 ground truths (G differs from
    # G_max on two images, the offsets are 0, 1, 4): a box over the whole frame on two images, two near-duplicates with different labels, a box of
    # 6 x 5 px (about 4 x 3.4 px in the network: narrower than one cell of map 0, mask-target grid 1), an all-one and an all-zero mask
    'mixed': dict(frames=[(90, 60), (60, 90), (70, 70)], resize=(48, 64), seeds=(34, 44, 8),
                  gt=[[(0, 0, 60, 90, 1)],
                      [(10, 10, 50, 40, 1), (12, 9, 52, 42, 2), (60, 30, 88, 58, 1, 1.0)],
                      [(0, 0, 70, 70, 2), (40, 20, 46, 25, 1), (5, 5, 35, 30, 1, 0.0), (30, 35, 65, 66, 2), (3, 40, 28, 68, 1)]]),
}


def frames(case):
    rng = np.random.RandomState(CASES[case]['seeds'][0])
    return [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in CASES[case]['frames']]


def targets(case):
    """boxes (G,4) float32, labels (G) int64, masks (G,h,w) uint8: the box filled to the ground truth's share (MASK_FILL: 80 %)"""
    c = CASES[case]
    rng = np.random.RandomState(c['seeds'][1])
    out = []
    for (h, w), gts in zip(c['frames'], c['gt']):
        boxes = np.array([g[:4] for g in gts], np.float32)
        masks = np.zeros((len(gts), h, w), np.uint8)
        for m, (x1, y1, x2, y2), g in zip(masks, boxes.astype(int), gts):
            m[y1:y2, x1:x2] = rng.uniform(0, 1, (y2 - y1, x2 - x1)) < (g[5] if len(g) > 5 else MASK_FILL)     # uniform < 1 always, < 0 never
        out.append(dict(boxes=boxes, labels=np.array([g[4] for g in gts], np.int64), masks=masks))
    return out


def keys(case, n_anchors):
    c = CASES[case]
    rng = np.random.RandomState(c['seeds'][2])
    B, G_max = len(c['frames']), max(len(g) for g in c['gt'])
    return dict(rpn=rng.randint(0, 2 ** 31 - 1, (B, n_anchors)).astype(np.int32), roi=rng.randint(0, 2 ** 31 - 1, (B, TOP_N + G_max)).astype(np.int32))


def feature_sizes(padded_size):
    """the five maps' sizes: stem and pool halve twice, every later stage and the pool level once more"""
    half = lambda s: ((s[0] - 1) // 2 + 1, (s[1] - 1) // 2 + 1)
    out = [half(half(tuple(padded_size)))]
    for _ in range(N_STAGES):
        out.append(half(out[-1]))
    return out


def padded_size(case):
    c = CASES[case]
    return detin_ref.padded_size([detin_ref.network_size(h, w, min(c['resize']), max(c['resize'])) for h, w in c['frames']])


def n_anchors(padded_size):
    return len(RATIOS) * sum(h * w for h, w in feature_sizes(padded_size))


def padded(parts, per_image, fill, dtype):
    """[(n_b, ...)] -> (B per_image, ...) rows, image b's first n_b real and the rest `fill`"""
    out = np.full((len(parts) * per_image,) + np.asarray(parts[0]).shape[1:], fill, dtype)
    for b, p in enumerate(parts):
        out[b * per_image:b * per_image + len(p)] = p
    return torch.from_numpy(out)


def real_rows(inp, key, counts):
    """the padded rows of inp[key] -> per image its real rows"""
    per = int(inp[key].shape[0]) // len(inp['net_sizes'])
    return [inp[key][b * per:b * per + int(c)] for b, c in enumerate(inp[counts])]


def check_reach(case, inp, kinks):
    """What each case was chosen to reach, asserted on detector_chain_ref.Chain's inputs (the twins' on the CPU, the device's own on the GPU) and on
    the kinks of a float64 step over them; prints a summary first."""
    B = len(inp['net_sizes'])
    positives, backgrounds = [int(c) for c in inp['pos_counts']], [int((l == 0).sum()) for l in real_rows(inp, 'roi_labels', 'roi_counts')]
    box_levels, mask_levels = ([sorted(set(r.tolist())) for r in real_rows(inp, k, c)] for k, c in (('roi_levels', 'roi_counts'), ('pos_levels', 'pos_counts')))
    matched = [r.tolist() for r in real_rows(inp, 'pos_matched', 'pos_counts')]
    print(f'{case}: images {tuple(inp["images"].shape)}, network sizes {inp["net_sizes"]}, ground truths {[len(g) for g in inp["gt_boxes"]]}, sampled RoIs '
          f'{[int(c) for c in inp["roi_counts"]]}, positives {positives}, background rows {backgrounds}, levels of the box path {box_levels}, of the mask path '
          f'{mask_levels} with {torch.bincount(torch.cat(real_rows(inp, "pos_levels", "pos_counts")).long(), minlength=4).tolist()} RoIs')
    assert B == len(CASES[case]['frames']) and tuple(inp['padded_size']) == tuple(padded_size(case))
    assert min(positives) >= 2 and min(backgrounds) >= 1
    across = lambda levels: set().union(*levels)
    if case == 'small':
        assert across(box_levels) == across(mask_levels) == {0}
    if case == 'two-levels':
        assert len(across(box_levels)) >= 2 and len(across(mask_levels)) >= 2 and tuple(inp['padded_size']) == (160, 224)
        assert all(len(g) == 1 and float(min(g[0, 2] - g[0, 0], g[0, 3] - g[0, 1])) > 130 for g in inp['gt_boxes'])
    if case == 'four-levels':
        assert B == 1 and tuple(inp['padded_size']) == (480, 640) == tuple(inp['net_sizes'][0])
        assert across(box_levels) == across(mask_levels) == {0, 1, 2, 3}
    if case == 'mixed':
        assert len(set(inp['net_sizes'])) == B == 3 and [len(g) for g in inp['gt_boxes']] == [1, 3, 5] == [len(g) for g in inp['gt_masks']]
        gts = CASES[case]['gt']
        tiny = [(b, i) for b in range(B) for i, g in enumerate(gts[b]) if min(g[2] - g[0], g[3] - g[1]) < 8]
        filled = {fill: [(b, i) for b in range(B) for i, g in enumerate(gts[b]) if len(g) > 5 and g[5] == fill] for fill in (0.0, 1.0)}
        assert len(tiny) == len(filled[0.0]) == len(filled[1.0]) == 1
        (tb, ti), (zb, zi), (ob, oi) = tiny[0], filled[0.0][0], filled[1.0][0]
        assert ti in matched[tb] and zi in matched[zb] and oi in matched[ob]       # each of them is the match of a sampled positive
        box = inp['gt_boxes'][tb][ti]
        assert float(box[2] - box[0]) * 0.25 < 1.25 and float(box[3] - box[1]) * 0.25 < 1.25       # on map 0 about one cell: RoIAlign's max(extent, 1)
        assert not inp['gt_masks'][zb][zi].any()
        x1, y1, x2, y2 = (float(v) for v in inp['gt_boxes'][ob][oi])
        assert inp['gt_masks'][ob][oi][math.ceil(y1) + 1:math.floor(y2) - 1, math.ceil(x1) + 1:math.floor(x2) - 1].all()
        grids = dict(kinks)['mask target grid']                                    # (2, the real positives), image after image
        first = sum(positives[:tb])
        of_tiny = [first + r for r, m in enumerate(matched[tb]) if m == ti]
        assert int(grids.min()) == 1 and bool((grids[:, of_tiny] == 1).all())
        full = [bool(((g[:, 2] - g[:, 0] >= w - 1) & (g[:, 3] - g[:, 1] >= h - 1)).any()) for g, (h, w) in zip(inp['gt_boxes'], inp['net_sizes'])]
        assert sum(full) >= 2                                                      # a ground truth over the whole frame on two images


@functools.lru_cache(maxsize=None)
def cpu_inputs(case):
    """detector_chain_ref.Chain's inputs from the twins on the CPU: detin_ref's transform, the float32 torch.nn trunk and RPN head for the values
    the decisions read, then dettrain_ref's match and samplers, detpre_ref's proposals and level mapper.  Computed once, handed out unchanged."""
    c = CASES[case]
    t = detin_ref.transform([f.transpose(2, 0, 1) for f in frames(case)], targets(case), min(c['resize']), max(c['resize']))
    nets, pad, tg = t['net_sizes'], t['padded_size'], t['targets']
    sd = tc.detector_weights()
    with torch.no_grad():
        maps = tc.torch_trunk(sd)(torch.from_numpy(t['images']))
        objectness, deltas = hc.torch_heads(sd)[0](maps)
    objectness, deltas = [o.numpy() for o in objectness], [d.numpy() for d in deltas]
    gt = [np.asarray(x['boxes'], np.float32) for x in tg]
    assert tuple(pad) == tuple(padded_size(case))
    k = keys(case, n_anchors(pad))
    rpn = tr.rpn_loss(objectness, deltas, gt, pad, SIZES, RATIOS, k['rpn'], RPN_BATCH)
    props = pre.proposals(objectness, deltas, nets, pad, SIZES, RATIOS, pre_nms_top_n=TOP_N, post_nms_top_n=TOP_N)
    G_max = max(len(g) for g in gt)
    smp = [tr.roi_samples(props[b]['boxes'], gt[b], tg[b]['labels'], k['roi'][b], TOP_N, G_max, ROI_BATCH) for b in range(len(gt))]
    src = [np.where(s['idx'] < len(p['boxes']), np.append(p['src'], -1)[np.minimum(s['idx'], len(p['boxes']))], -1) for s, p in zip(smp, props)]
    inp = dict(images=torch.from_numpy(t['images']), net_sizes=[tuple(n) for n in nets], padded_size=tuple(pad),
               gt_boxes=[torch.from_numpy(g) for g in gt], gt_labels=[torch.from_numpy(np.asarray(x['labels'])) for x in tg],
               gt_masks=[torch.from_numpy(np.ascontiguousarray(x['masks'])) for x in tg],
               anchors=torch.from_numpy(pre.anchors([m.shape[2:] for m in maps], pad, SIZES, RATIOS)),
               rpn_matched=torch.from_numpy(rpn['matched']), rpn_samp_idx=padded(rpn['sampled'], RPN_BATCH, -1, np.int64).reshape(len(gt), RPN_BATCH),
               rpn_samp_count=torch.tensor([len(s) for s in rpn['sampled']]),
               roi_boxes=padded([s['boxes'] for s in smp], ROI_BATCH, 0, np.float32), roi_labels=padded([s['labels'] for s in smp], ROI_BATCH, -1, np.int64),
               roi_matched=padded([s['matched'] for s in smp], ROI_BATCH, 0, np.int64), roi_counts=torch.tensor([len(s['idx']) for s in smp]),
               roi_src=padded(src, ROI_BATCH, -1, np.int64),
               pos_boxes=padded([s['pos_boxes'] for s in smp], ROI_POSITIVES, 0, np.float32),
               pos_labels=padded([s['pos_labels'] for s in smp], ROI_POSITIVES, 0, np.int64),
               pos_matched=padded([s['pos_matched'] for s in smp], ROI_POSITIVES, 0, np.int64), pos_counts=torch.tensor([len(s['pos_idx']) for s in smp]))
    inp['roi_levels'] = torch.from_numpy(pre.map_levels(inp['roi_boxes'].numpy(), 2, 5))
    inp['pos_levels'] = torch.from_numpy(pre.map_levels(inp['pos_boxes'].numpy(), 2, 5))
    return inp
