"""The cases that tests/test_detector_chain_host.py (CPU) and tests/test_detector_chain.py (GPU) share: seeded frames, targets and sampler keys
for one training step of the narrow detector of dettrunk_case.detector_weights(), and the inputs of detector_chain_ref.Chain taken from the
twins' chain on the CPU (the GPU test takes them from the device run instead).  The seeds were chosen on the CPU so that the float64 graph and
its float32 replica take the same side at every kink (test_detector_chain_host.py keeps that check)."""
import functools

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

# name -> frame sizes (h, w), input_resize, seeds of the frames / the masks / the keys, ground truths per frame (x1, y1, x2, y2, label)
CASES = {
    # tests/test_detector_trunk_backward.py's end-to-end frames and targets: 64 x 64 after padding, every RoI on level 0
    'small': dict(frames=tc.E2E_FRAMES, resize=(48, 64), seeds=(31, 41, 5),
                  gt=[[(3, 4, w - 12, h - 9, 1), (w // 3, h // 4, w - 4, h - 3, 2)] for h, w in tc.E2E_FRAMES]),
    # 160 x 224 after the resize, one ground truth per frame whose sides exceed 130 px there: the smallest frames at which the level mapper
    # leaves level 0 (sqrt(area) >= 112)
    'two-levels': dict(frames=[(120, 168), (150, 200)], resize=(160, 224), seeds=(32, 42, 6),
                       gt=[[(0, 0, 118, 103, 1)], [(0, 24, 127, 150, 2)]]),
}


def frames(case):
    rng = np.random.RandomState(CASES[case]['seeds'][0])
    return [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in CASES[case]['frames']]


def targets(case):
    """boxes (G,4) float32, labels (G) int64, masks (G,h,w) uint8: the box filled to 80 %"""
    c = CASES[case]
    rng = np.random.RandomState(c['seeds'][1])
    out = []
    for (h, w), gts in zip(c['frames'], c['gt']):
        boxes = np.array([g[:4] for g in gts], np.float32)
        masks = np.zeros((len(gts), h, w), np.uint8)
        for m, (x1, y1, x2, y2) in zip(masks, boxes.astype(int)):
            m[y1:y2, x1:x2] = rng.uniform(0, 1, (y2 - y1, x2 - x1)) < 0.8
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
