"""The differentiable part of detector_losses_from_frames (DESIGN.md sections 21 to 25) in plain torch: tensor operations, torch.nn.functional
and autograd, float64 by default.  No twin is imported and no adjoint is written by hand: every gradient is autograd's.  The trunk and the heads
are the torch.nn modules of dettrunk_case.torch_trunk and dethead_case.torch_heads; everything between them is stated here.

Inputs (`inp`, a dict of CPU tensors in the device's padded layout) are the discrete and the detached quantities of a training step, which the
caller takes from the run it checks, so that a float32 / float64 flip of a decision cannot look like a gradient error:
  images (B,3,Hp,Wp) float32, net_sizes [(h,w)], padded_size (Hp,Wp); gt_boxes [(G_b,4)], gt_labels [(G_b)], gt_masks [(G_b,h_b,w_b) uint8];
  anchors (N,4); rpn_matched (B,N), rpn_samp_idx (B,bs), rpn_samp_count (B); roi_boxes (B rows,4), roi_labels, roi_matched, roi_levels (B rows),
  roi_counts (B); pos_boxes (B n,4), pos_labels, pos_matched, pos_levels (B n), pos_counts (B); and, for one mutation only, roi_src (B rows): the
  anchor a sampled proposal was decoded from (-1: a ground truth).
Everything else is computed here: the trunk, the FPN and the pool level, the three heads, both box encodes, the five losses, the multi-scale
RoIAlign (torchvision 0.4.2: aligned=False, a sample outside [-1, size] is 0, a coordinate <= 0 is 0, floor / gather / multiply) and the mask
targets (the same RoIAlign over the uint8 masks at scale 1 with the adaptive grid ceil(max(extent, 1) / M)).

dtype=torch.float32 runs the same graph in float32.  storage='bfloat16' puts a straight-through rounding at section 30's storage points.
mutate=<one of MUTATIONS> is for the tests of this file's own teeth.  Chain.kinks lists, after a forward, the side taken at every ReLU, L1 sign,
smooth-L1 branch, RoIAlign floor and adaptive grid: two runs took the same path when these are equal."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import dethead_case as hc
import dettrunk_case as tc

LOSS_KEYS = ('loss_objectness', 'loss_rpn_box_reg', 'loss_classifier', 'loss_box_reg', 'loss_mask')
RPN_WEIGHTS, ROI_WEIGHTS = (1.0, 1.0, 1.0, 1.0), (10.0, 10.0, 5.0, 5.0)
XFORM_CLIP = math.log(1000.0 / 16)
BOUNDARY = 1e-4                      # cells; float32's rounding of a sample position here is below 1e-5
MUTATIONS = ('mask_over_padded_rows', 'pool_detached', 'proposals_differentiable', 'sampling_ratio_1', 'level1_reads_map0', 'rpn_box_over_positives',
             'level2_reads_map1', 'level3_reads_map2', 'gt_rows_at_gmax_stride')
LEVEL_MUTATIONS = {f'level{l}_reads_map{l - 1}': l for l in (1, 2, 3)}             # the rows of level l read the map below with level l's scale
HEAD_PREFIXES = ('rpn.head', 'roi_heads.box_head', 'roi_heads.box_predictor', 'roi_heads.mask_head', 'roi_heads.mask_predictor')
# the head modules whose input is a ReLU's output
AFTER_RELU = ('rpn.head.cls_logits', 'roi_heads.box_head.fc7', 'roi_heads.box_predictor.cls_score', 'roi_heads.mask_head.mask_fcn2',
              'roi_heads.mask_head.mask_fcn3', 'roi_heads.mask_head.mask_fcn4', 'roi_heads.mask_predictor.conv5_mask',
              'roi_heads.mask_predictor.mask_fcn_logits')


def bf16(x):
    return x.to(torch.bfloat16).to(x.dtype)


class _Stored(torch.autograd.Function):
    """straight through a bfloat16 store: the value rounded on the way forward (fwd), the gradient on the way back (bwd)"""

    @staticmethod
    def forward(ctx, x, fwd, bwd):
        ctx.bwd = bwd
        return bf16(x) if fwd else x.clone()

    @staticmethod
    def backward(ctx, g):
        return (bf16(g) if ctx.bwd else g), None, None


# ---- box coder ---------------------------------------------------------------------------------------------------------------------------
def encode(reference, proposals, weights):
    """BoxCoder.encode_single"""
    wx, wy, ww, wh = weights
    ew, eh = proposals[:, 2] - proposals[:, 0], proposals[:, 3] - proposals[:, 1]
    ecx, ecy = proposals[:, 0] + 0.5 * ew, proposals[:, 1] + 0.5 * eh
    gw, gh = reference[:, 2] - reference[:, 0], reference[:, 3] - reference[:, 1]
    gcx, gcy = reference[:, 0] + 0.5 * gw, reference[:, 1] + 0.5 * gh
    return torch.stack([wx * (gcx - ecx) / ew, wy * (gcy - ecy) / eh, ww * torch.log(gw / ew), wh * torch.log(gh / eh)], 1)


def decode(deltas, anchors):
    """BoxCoder.decode_single with weights 1 (only the mutation that lets a gradient through the proposals uses it)"""
    w, h = anchors[:, 2] - anchors[:, 0], anchors[:, 3] - anchors[:, 1]
    cx, cy = anchors[:, 0] + 0.5 * w, anchors[:, 1] + 0.5 * h
    pcx, pcy = deltas[:, 0] * w + cx, deltas[:, 1] * h + cy
    pw, ph = torch.exp(deltas[:, 2].clamp(max=XFORM_CLIP)) * w, torch.exp(deltas[:, 3].clamp(max=XFORM_CLIP)) * h
    return torch.stack([pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph], 1)


# ---- RoIAlign ----------------------------------------------------------------------------------------------------------------------------
def _axis(lo, hi, scale, P, g, size, kinks, name):
    """one axis of n boxes -> valid (n, P g) bool, low and high index (n, P g), weight of the high tap (n, P g)"""
    start, end = lo * scale, hi * scale
    extent = end - start
    extent = torch.where(extent > 1, extent, torch.ones_like(extent))              # max(extent, 1)
    bin_ = (extent / P)[:, None]
    p = torch.arange(P, dtype=lo.dtype).repeat_interleave(g)[None]
    i = torch.arange(g, dtype=lo.dtype).repeat(P)[None]
    v = (start[:, None] + p * bin_) + ((i + 0.5) * bin_) / g
    valid = (v >= -1) & (v <= size)
    v = torch.where(v <= 0, torch.zeros_like(v), v)
    floor = v.detach().floor()
    if kinks is not None:
        # a sample within BOUNDARY of a whole number sits ON the border of two cells and belongs to both: the interpolation is continuous there and
        # the boxes are constants, so neither side is a decision.  It is recorded as that border (a half), every other sample as its cell.
        nearest = v.detach().round()
        side = torch.where((v.detach() - nearest).abs() < BOUNDARY, nearest - 0.5, floor)
        kinks.append((name + ' inside', valid))
        kinks.append((name + ' floor', torch.where(valid, side, torch.zeros_like(side)).double()))
    low = floor.clamp(0, size - 1).long()
    top = low >= size - 1
    high = torch.where(top, low, low + 1)
    v = torch.where(top, low.to(v.dtype), v)
    return valid, low, high, v - low.to(v.dtype)


def roi_align(feat, im, boxes, scale, P, gh, gw, kinks=None, name='roi_align'):
    """feat (B,C,H,W), im (n) long, boxes (n,4) -> (n,C,P,P): the mean over gh x gw bilinear samples per bin"""
    n, (C, H, W) = int(boxes.shape[0]), feat.shape[1:]
    vy, y0, y1, ly = _axis(boxes[:, 1], boxes[:, 3], scale, P, gh, H, kinks, name + ' y')
    vx, x0, x1, lx = _axis(boxes[:, 0], boxes[:, 2], scale, P, gw, W, kinks, name + ' x')
    b = im[:, None, None]
    Y0, Y1, X0, X1 = y0[:, :, None], y1[:, :, None], x0[:, None, :], x1[:, None, :]
    LY, LX = ly[:, :, None, None], lx[:, None, :, None]
    HY, HX = 1 - LY, 1 - LX
    v = HY * HX * feat[b, :, Y0, X0] + HY * LX * feat[b, :, Y0, X1] + LY * HX * feat[b, :, Y1, X0] + LY * LX * feat[b, :, Y1, X1]      # (n, P gh, P gw, C)
    v = v * (vy[:, :, None] & vx[:, None, :])[..., None].to(v.dtype)
    return (v.reshape(n, P, gh, P, gw, C).sum((2, 4)) / (gh * gw)).permute(0, 3, 1, 2)


def infer_scales(maps, net_sizes):
    """MultiScaleRoIAlign.setup_scales: 2^round(log2(H_l / the largest image height))"""
    top = max(h for h, _ in net_sizes)
    return [2.0 ** round(math.log2(float(m.shape[2]) / top)) for m in maps]


def multiscale_roi_align(maps, scales, boxes, im, levels, P, g, kinks=None, wrong_level=None, name='roi_align'):
    """the row's level selects the map and the scale -> (n,C,P,P) (wrong_level: the mutation whose rows of that level read the map below)"""
    out = maps[0].new_zeros((int(boxes.shape[0]), int(maps[0].shape[1]), P, P))
    for l in range(len(maps)):
        rows = torch.nonzero(levels == l).reshape(-1)
        if rows.numel():
            feat = maps[l - 1] if l == wrong_level else maps[l]
            out[rows] = roi_align(feat, im[rows], boxes[rows], scales[l], P, g, g, kinks, f'{name} level {l}')
    return out


def mask_targets(masks, boxes, im, matched, M, dtype, kinks=None):
    """project_masks_on_boxes: masks [(G_b,h_b,w_b) uint8], boxes (n,4), im, matched (n) long -> (n,M,M)"""
    ext_h, ext_w = boxes[:, 3] - boxes[:, 1], boxes[:, 2] - boxes[:, 0]
    grid = lambda e: torch.ceil(torch.where(e > 1, e, torch.ones_like(e)) / M).long().clamp(min=1)
    gh, gw = grid(ext_h), grid(ext_w)
    if kinks is not None:
        kinks.append(('mask target grid', torch.stack([gh, gw])))
    out = boxes.new_zeros((int(boxes.shape[0]), M, M))
    for key in sorted({(int(b), int(a), int(c)) for b, a, c in zip(im, gh, gw)}):
        rows = torch.nonzero((im == key[0]) & (gh == key[1]) & (gw == key[2])).reshape(-1)
        planes = masks[key[0]].to(dtype)[None]                                       # one "image" whose channels are the ground truths
        all_gt = roi_align(planes, torch.zeros_like(rows), boxes[rows], 1.0, M, key[1], key[2], kinks, f'mask target image {key[0]} grid {key[1]}x{key[2]}')
        out[rows] = all_gt[torch.arange(rows.numel()), matched[rows]]
    return out


# ---- the five losses ---------------------------------------------------------------------------------------------------------------------
def rpn_losses(logits, deltas, anchors, gt, matched, samp_idx, samp_count, kinks=None, over_positives=False):
    """logits (B,N), deltas (B,N,4) in the anchors' order; matched (B,N): >= 0 the ground truth of a positive; samp_idx (B,bs), its first
    samp_count[b] real -> BCE-with-logits over the sampled, the L1 sum over the sampled positives / the sampled"""
    x, y, diff = [], [], []
    for b in range(int(logits.shape[0])):
        idx = samp_idx[b, :int(samp_count[b])]
        m = matched[b, idx]
        x.append(logits[b, idx]), y.append((m >= 0).to(logits.dtype))
        diff.append(deltas[b, idx[m >= 0]] - encode(gt[b][m[m >= 0]], anchors[idx[m >= 0]], RPN_WEIGHTS))
    x, y, diff = torch.cat(x), torch.cat(y), torch.cat(diff)
    if kinks is not None:
        kinks.append(('rpn l1 sign', diff > 0))
    return F.binary_cross_entropy_with_logits(x, y), diff.abs().sum() / (diff.shape[0] if over_positives else x.numel())


def fastrcnn_losses(class_logits, box_regression, labels, targets, kinks=None):
    """the real rows only: class_logits (n,K), box_regression (n,4K), labels (n) long, targets (n,4) -> cross entropy, smooth-L1 (beta 1) over
    the label's four columns of the foreground rows / n"""
    n, fg = int(labels.shape[0]), labels > 0
    own_columns = box_regression.reshape(n, -1, 4)[fg, labels[fg]]
    if kinks is not None:
        kinks.append(('smooth l1 branch', (own_columns - targets[fg]).abs() < 1)), kinks.append(('smooth l1 sign', own_columns > targets[fg]))
    return F.cross_entropy(class_logits, labels), F.smooth_l1_loss(own_columns, targets[fg], reduction='sum', beta=1.0) / n


def mask_loss(mask_logits, labels, wanted, n_padded=None):
    """the real rows only: mask_logits (n,K,M,M), labels (n) long, wanted (n,M,M) -> BCE-with-logits on the label's channel, averaged over n M^2
    (n_padded: the mutation that divides by all padded rows)"""
    own_channel = mask_logits[torch.arange(int(labels.shape[0])), labels]
    if n_padded is not None:
        return F.binary_cross_entropy_with_logits(own_channel, wanted, reduction='sum') / (n_padded * wanted.shape[-1] * wanted.shape[-2])
    return F.binary_cross_entropy_with_logits(own_channel, wanted)


# ---- the chain ---------------------------------------------------------------------------------------------------------------------------
class Chain:
    """the detector of a state dict under torchvision's names as torch.nn modules in `dtype`, with the device's trainable set: the conv weights
    of body.layer{train_from_stage}.., the FPN and the heads"""

    def __init__(self, sd, train_from_stage=2, dtype=torch.float64, storage=None, mutate=None):
        if storage not in (None, 'bfloat16'):
            raise ValueError(f'storage is None or bfloat16, got {storage!r}')
        if mutate is not None and mutate not in MUTATIONS:
            raise ValueError(f'unknown mutation {mutate!r}')
        self.dtype, self.storage, self.mutate, self.kinks = dtype, storage, mutate, []
        sd = {k: np.asarray(v) for k, v in sd.items()}
        self.trunk = tc.torch_trunk(sd).to(dtype)
        self.heads = dict(zip(HEAD_PREFIXES, hc.torch_heads(sd, dtype)))
        self.params = {}
        for k, p in self.trunk.named_parameters():
            stage = int(k.split('.')[1][5:]) if k.startswith('body.layer') else None
            if k.startswith('fpn.') or (stage is not None and stage >= train_from_stage):
                self.params['backbone.' + k] = p.requires_grad_(True)
        for prefix, m in self.heads.items():
            for k, p in m.named_parameters():
                self.params[f'{prefix}.{k}'] = p.requires_grad_(True)
            for k, sub in m.named_modules():
                if f'{prefix}.{k}' in AFTER_RELU:
                    sub.register_forward_pre_hook(lambda _, args, name=f'{prefix}.{k}': self.kinks.append((name, args[0] > 0)))

    def named_parameters(self):
        return dict(self.params)

    def zero_grad(self):
        for p in self.params.values():
            p.grad = None

    # ---- the trunk, layer by layer over the module's own submodules (storage=None: the module's forward, value for value) ----
    def _stored(self, x, fwd=True, bwd=True):
        return _Stored.apply(x, fwd, bwd) if self.storage else x

    def _conv(self, m, x):
        return F.conv2d(x, self._stored(m.weight, bwd=False), m.bias, m.stride, m.padding)      # .grad stays float32: the master weights

    def _relu(self, name, x):
        self.kinks.append((name, x > 0))
        return self._stored(torch.relu(x))

    def trunk_forward(self, images):
        body, fpn = self.trunk.body, self.trunk.fpn
        x = self._stored(images)
        x = self._stored(torch.relu(body.bn1(self._conv(body.conv1, x))))           # the stem is a constant: its ReLU and the pool are no kinks of the gradient
        x = F.max_pool2d(x, 3, 2, 1)
        feats = []
        for s in range(1, body.n + 1):
            for i, blk in enumerate(getattr(body, f'layer{s}')):
                name = f'body.layer{s}.{i}'
                a = self._relu(name + '.conv1', blk.bn1(self._conv(blk.conv1, x)))
                b = self._relu(name + '.conv2', blk.bn2(self._conv(blk.conv2, a)))
                c = blk.bn3(self._conv(blk.conv3, b))
                short = x if blk.downsample is None else self._stored(blk.downsample[1](self._conv(blk.downsample[0], x)))
                x = self._relu(name, c + short)
            feats.append(x)
        last = self._stored(self._conv(fpn.inner_blocks[-1], feats[-1]))
        out = [self._stored(self._conv(fpn.layer_blocks[-1], last), fwd=False)]       # the maps are float32; the gradient that arrives is packed
        for l in range(len(feats) - 2, -1, -1):
            lateral = self._conv(fpn.inner_blocks[l], feats[l])
            last = self._stored(lateral + F.interpolate(last, size=lateral.shape[-2:], mode='nearest'))
            out.insert(0, self._stored(self._conv(fpn.layer_blocks[l], last), fwd=False))
        return out + [F.max_pool2d(out[-1], 1, 2, 0)]

    # ---- images -> the five losses ----
    def losses(self, inp):
        dt, kinks = self.dtype, self.kinks
        kinks.clear()
        long = lambda k: inp[k].long()
        images = inp['images'].to(dt)
        B = int(images.shape[0])
        maps = self.trunk_forward(images)
        if self.mutate == 'pool_detached':
            maps[4] = maps[4].detach()
        self.maps = maps
        for m in maps:
            if m.requires_grad:
                m.retain_grad()
        rpn, box_head, predictor, mask_head, mask_predictor = self.heads.values()
        objectness, deltas = rpn(maps)
        A = int(objectness[0].shape[1])
        logits = torch.cat([o.permute(0, 2, 3, 1).reshape(B, -1) for o in objectness], 1)                     # (B, N): (y W + x) A + a within a level
        deltas = torch.cat([d.reshape(B, A, 4, *d.shape[2:]).permute(0, 3, 4, 1, 2).reshape(B, -1, 4) for d in deltas], 1)
        anchors = inp['anchors'].to(dt)
        gt = [g.to(dt) for g in inp['gt_boxes']]
        if self.mutate == 'gt_rows_at_gmax_stride':
            # the planted mistake: the ground truths lie one after another, image b's from offset[b] on; row b G_max + m is read instead of
            # offset[b] + m (modulo the table's length, to stay inside it).  Nothing moves when every image holds G_max ground truths
            table, G_max = torch.cat(gt), max(int(g.shape[0]) for g in gt)
            gt = [table[(b * G_max + torch.arange(G_max)) % int(table.shape[0])] for b in range(B)]

        loss_objectness, loss_rpn_box_reg = rpn_losses(logits, deltas, anchors, gt, long('rpn_matched'), long('rpn_samp_idx'), long('rpn_samp_count'), kinks,
                                                       self.mutate == 'rpn_box_over_positives')

        # the box branch over the real rows
        roi_maps, g = maps[:4], 1 if self.mutate == 'sampling_ratio_1' else 2
        scales = infer_scales(roi_maps, inp['net_sizes'])
        wrong_map = LEVEL_MUTATIONS.get(self.mutate)
        rows, im = self._real_rows(long('roi_counts'), int(inp['roi_boxes'].shape[0]) // B)
        boxes, labels = inp['roi_boxes'][rows].to(dt), long('roi_labels')[rows]
        if self.mutate == 'proposals_differentiable':
            src = long('roi_src')[rows]
            own = src >= 0
            size = torch.tensor([[w, h, w, h] for h, w in inp['net_sizes']], dtype=dt)[im[own]]
            decoded = torch.minimum(decode(deltas[im[own], src[own]], anchors[src[own]]).clamp(min=0), size)
            assert float((decoded.detach() - boxes[own]).abs().max()) < 0.05, 'roi_src does not name the anchors of the sampled proposals'
            boxes = boxes.clone()
            boxes[own] = decoded
        feats = multiscale_roi_align(roi_maps, scales, boxes, im, long('roi_levels')[rows], 7, g, kinks, wrong_map, 'box roi_align')
        class_logits, box_regression = predictor(box_head(feats))
        gt_of_row = torch.stack([gt[int(b)][int(m)] for b, m in zip(im, long('roi_matched')[rows])])
        loss_classifier, loss_box_reg = fastrcnn_losses(class_logits, box_regression, labels, encode(gt_of_row, boxes, ROI_WEIGHTS), kinks)

        # the mask branch over the sampled positives
        n_pad = int(inp['pos_boxes'].shape[0])
        rows, im = self._real_rows(long('pos_counts'), n_pad // B)
        boxes, labels = inp['pos_boxes'][rows].to(dt), long('pos_labels')[rows]
        feats = multiscale_roi_align(roi_maps, scales, boxes, im, long('pos_levels')[rows], 14, g, kinks, wrong_map, 'mask roi_align')
        mask_logits = mask_predictor(mask_head(feats))
        wanted = mask_targets(inp['gt_masks'], boxes, im, long('pos_matched')[rows], int(mask_logits.shape[-1]), dt, kinks)
        loss_mask = mask_loss(mask_logits, labels, wanted, n_pad if self.mutate == 'mask_over_padded_rows' else None)
        self.mask_targets = wanted
        return dict(zip(LOSS_KEYS, (loss_objectness, loss_rpn_box_reg, loss_classifier, loss_box_reg, loss_mask)))

    @staticmethod
    def _real_rows(counts, per_image):
        """padded rows: image b owns rows [b per_image, (b + 1) per_image), its first counts[b] are real -> the real rows, their images"""
        rows = torch.cat([b * per_image + torch.arange(int(c)) for b, c in enumerate(counts)])
        return rows, rows // per_image

    def step(self, inp, only=None):
        """one forward and one backward of the sum of the losses (only: of the named ones) -> losses, {name: gradient}, the gradients at the maps"""
        self.zero_grad()
        losses = self.losses(inp)
        sum(v for k, v in losses.items() if only is None or k in only).backward()
        grads = {k: p.grad.detach().clone() for k, p in self.params.items() if p.grad is not None}
        return {k: v.detach() for k, v in losses.items()}, grads, [None if m.grad is None else m.grad.detach().clone() for m in self.maps]


def kink_disagreements(a, b):
    """two kink lists -> [(name, elements on another side)] of the entries that differ (a different structure counts whole)"""
    if [k for k, _ in a] != [k for k, _ in b]:
        return [('structure', max(len(a), len(b)))]
    out = []
    for (name, u), (_, v) in zip(a, b):
        if u.shape != v.shape:
            out.append((name, max(u.numel(), v.numel())))
        elif not torch.equal(u, v):
            out.append((name, int((u != v).sum())))
    return out
