"""The detector's input side on the device: torchvision 0.4.2's GeneralizedRCNNTransform -- the first thing model(images, targets) does, in
the reference's Detector.get_detections (cosypose/integrated/detector.py) as in h_maskrcnn of its training -- for uint8 frames.  DESIGN.md
section 25 holds the definition; csrc/kernels_detin.hip the kernel; tests/detin_ref.py the numpy twin.

    inp = detector_input(frames, targets)                       # raw uint8 frames of any sizes, CHW or HWC, read in place
    feats = backbone(inp.images)
    dets = detections_from_features(feats, rpn_head, box_head, mask_head, inp.net_sizes, inp.padded_size, inp.original_sizes, names)
    loss = detector_losses(feats, rpn_head, box_head, mask_head, inp.targets, inp.net_sizes, inp.padded_size)

or detections_from_frames / detector_losses_from_frames, which are exactly these lines.

A frame is normalised ((u / 255 - mean) / std, a 3 x 256 table), resized so that its short side reaches min_size unless the long side
would pass max_size (float32 bilinear interpolation with half-pixel centres), and written into one batch whose sides are multiples of
size_divisible, +0.0 outside the image; the boxes of its target are scaled and its masks resized through nearest.  Everything that
divides -- the sizes (Python doubles, as torchvision has them), the table, the taps and weights of an axis, the nearest indices, the box
ratios -- is computed here on the host; a call uploads one buffer (the per-frame descriptors and the tables it uses) and makes ONE
launch, whatever the mix of sizes and however many masks.  There is no CPU path: tensors on the CPU are refused.
"""
import collections
import functools
import math
import sys
import types

import numpy as np

from . import _lib
from ._tables import TablePacker
from .frames import axis_offsets

F32 = np.float32
# cosy_detin_item_t
ITEM_DTYPE = np.dtype([('frame', '<u8'), ('sc', '<i8'), ('sy', '<i8'), ('sx', '<i8'), ('masks', '<u8'), ('masks_out', '<u8'), ('boxes', '<u8'),
                       ('boxes_out', '<u8'), ('h', '<i4'), ('w', '<i4'), ('nh', '<i4'), ('nw', '<i4'), ('xb', '<i4'), ('yb', '<i4'), ('xn', '<i4'),
                       ('yn', '<i4'), ('n_masks', '<i4'), ('n_boxes', '<i4'), ('rw', '<f4'), ('rh', '<f4'), ('flags', '<i4'), ('reserved', '<i4', (3,))])
assert ITEM_DTYPE.itemsize == 128
ONE_TAP = _lib.DETIN_ONE_TAP
MAX_UNITS = 65535                                            # frames + mask planes of one call: the grid's z dimension
MAX_ROWS = 524280                                            # 8 rows per workgroup, 65535 workgroups
IMAGE_MEAN, IMAGE_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

DetectorInput = collections.namedtuple('DetectorInput', 'images net_sizes padded_size original_sizes targets')
DetectorInput.__doc__ = """images (B,3,Hp,Wp) float32, +0.0 outside each image's (nh_i, nw_i); net_sizes [(nh_i, nw_i)], the net_sizes of
rpn_proposals / multiscale_roi_align / detector_losses; padded_size (Hp, Wp); original_sizes [(h_i, w_i)], the original_sizes of
detections_from_heads; targets None, or one dict per image: boxes scaled, masks resized, every other key the caller's own object"""


def network_size(h, w, min_size, max_size):
    """(nh, nw) of an h x w frame, in Python doubles exactly as torchvision 0.4.2 computes the scale factor and torch 1.3 the output size
    of interpolate(scale_factor=): floor(float(n) * s).  The floor's quirk is part of it: 49 x 70 at 32 / 64 gives nh = 31."""
    s = float(min_size) / float(min(h, w))
    if float(max(h, w)) * s > max_size:
        s = float(max_size) / float(max(h, w))
    return int(math.floor(float(h) * s)), int(math.floor(float(w) * s))


def padded_size(net_sizes, size_divisible=32):
    """(Hp, Wp) of batch_images: the largest height and width, each rounded up to a multiple of size_divisible"""
    d = int(size_divisible)
    return tuple(int(math.ceil(float(max(s[k] for s in net_sizes)) / d) * d) for k in (0, 1))


def box_ratios(h, w, nh, nw):
    """(rw, rh) of resize_boxes: a double quotient rounded once to float32, as a Python float times a float32 tensor is"""
    return F32(float(nw) / float(w)), F32(float(nh) / float(h))


@functools.lru_cache(maxsize=16)
def _pixel_table(mean, std):
    u = np.arange(256, dtype=F32)[None, :]
    m, s = np.asarray(mean, F32)[:, None], np.asarray(std, F32)[:, None]
    with np.errstate(all='ignore'):
        p = (((u / F32(255)).astype(F32) - m).astype(F32) / s).astype(F32)
    p.setflags(write=False)
    return p


def pixel_table(image_mean=IMAGE_MEAN, image_std=IMAGE_STD):
    """(3,256) float32: p_c(u) = ((float32(u) / 255f) - mean_c) / std_c, three IEEE operations with mean and std as float32; read-only"""
    try:
        mean, std = tuple(float(v) for v in image_mean), tuple(float(v) for v in image_std)
    except (TypeError, ValueError):
        raise ValueError(f'image_mean and image_std are three numbers each, got {image_mean!r} and {image_std!r}') from None
    if len(mean) != 3 or len(std) != 3:
        raise ValueError(f'image_mean and image_std are three numbers each, got {image_mean!r} and {image_std!r}')
    p = _pixel_table(mean, std)
    if not np.isfinite(p).all():
        raise ValueError(f'image_mean={image_mean!r}, image_std={image_std!r} give a pixel value that is not finite')
    return p


def _one_frame(i, t, torch):
    """-> (tensor, channel stride, row stride, pixel stride, h, w) of frame i, read in place"""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f'frame {i} must be a uint8 tensor, got {type(t)!r}')
    if t.dtype != torch.uint8:
        raise ValueError(f'frame {i} is {t.dtype}: only uint8 frames are served (a float frame would need torchvision\'s own transform)')
    if t.dim() != 3:
        raise ValueError(f'frame {i} must be (3,h,w) or (h,w,3), got {tuple(t.shape)}')
    s = t.stride()
    if t.shape[0] == 3:                                      # (3,h,w); a (3,w,3) tensor counts as this
        c, y, x = 0, 1, 2
    elif t.shape[2] == 3:
        y, x, c = 0, 1, 2
    else:
        raise ValueError(f'frame {i} must have 3 channels, first or last, got {tuple(t.shape)}')
    h, w = int(t.shape[y]), int(t.shape[x])
    if h < 1 or w < 1:
        raise ValueError(f'frame {i} has no pixels: {tuple(t.shape)}')
    if min(s) < 0:
        raise ValueError(f'frame {i} has a negative stride {tuple(s)}, which the kernel does not read')
    return t, int(s[c]), int(s[y]), int(s[x]), h, w


def _frames(frames, torch):
    if isinstance(frames, torch.Tensor):
        if frames.dim() != 4:
            raise ValueError(f'frames must be a list of uint8 tensors or one (B,3,h,w) / (B,h,w,3) uint8 tensor, got {tuple(frames.shape)}')
        frames = frames.unbind(0)
    elif not isinstance(frames, (list, tuple)):
        raise ValueError(f'frames must be a list of uint8 tensors or one 4-dimensional uint8 tensor, got {type(frames)!r}')
    if len(frames) == 0:
        raise ValueError('detector_input needs at least one frame')
    return [_one_frame(i, t, torch) for i, t in enumerate(frames)]


def _min_sizes(min_size, B):
    try:
        sizes = [int(min_size)] * B if not isinstance(min_size, (list, tuple, np.ndarray)) else [int(v) for v in min_size]
    except (TypeError, ValueError):
        raise ValueError(f'min_size must be an integer or one integer per image, got {min_size!r}') from None
    if len(sizes) != B or any(v < 1 for v in sizes):
        raise ValueError(f'min_size must be a positive integer or one per image ({B} images), got {min_size!r}')
    return sizes


def _check_targets(targets, parsed, torch):
    """-> [(boxes (G,4) float32 contiguous, masks (G,h,w) uint8 contiguous | None)]; nothing on the device is touched"""
    if not isinstance(targets, (list, tuple)) or not all(isinstance(t, dict) for t in targets):
        raise ValueError('targets must be a list of dicts (boxes and optionally masks), one per image')
    if len(targets) != len(parsed):
        raise ValueError(f'targets must hold one dict per image: {len(parsed)} images, got {len(targets)}')
    out = []
    for i, (t, (_, _, _, _, h, w)) in enumerate(zip(targets, parsed)):
        if 'keypoints' in t:
            raise NotImplementedError(f'targets[{i}] holds keypoints: key-point targets are not served (DESIGN.md section 25)')
        boxes = t.get('boxes')
        if not isinstance(boxes, torch.Tensor) or boxes.dtype != torch.float32 or boxes.dim() != 2 or boxes.shape[1] != 4:
            raise ValueError(f'targets[{i}] boxes must be a (G,4) float32 tensor')
        masks = t.get('masks')
        if masks is not None:
            if not isinstance(masks, torch.Tensor) or masks.dtype != torch.uint8 or masks.dim() != 3 or masks.shape[0] != boxes.shape[0]:
                raise ValueError(f'targets[{i}] masks must be a (G,h,w) uint8 tensor with one mask per box ({boxes.shape[0]})')
            if tuple(masks.shape[1:]) != (h, w):
                raise ValueError(f'targets[{i}] masks are {tuple(masks.shape[1:])}, its frame is {(h, w)}')
        out.append((boxes, masks))
    return out


def _empty(shape, dtype, device):
    """every output of a call is allocated here (the tests wrap it to put guards around the boxes and the masks)"""
    import torch
    return torch.empty(shape, dtype=dtype, device=device)


def detector_input(frames, targets=None, min_size=480, max_size=640, image_mean=IMAGE_MEAN, image_std=IMAGE_STD, size_divisible=32, out=None):
    """frames: a list of uint8 device tensors, each (3,h_i,w_i) or (h_i,w_i,3), of any mix of sizes, or one (B,3,h,w) / (B,h,w,3) tensor.
    They are read in place through their strides: a permute view or a slice of a larger tensor costs no copy.  (A (3,w,3) tensor is read as
    channels first.)  Float frames are refused.  min_size: an int, or one per image (a training loop that wants torchvision's
    random.choice(min_size) draws it itself).  targets[i]: a dict with boxes (G_i,4) float32 xyxy and optionally masks (G_i,h_i,w_i) uint8;
    G_i = 0 is allowed; a `keypoints` key raises NotImplementedError.  out: a contiguous float32 (B,3,Hp,Wp) device tensor to write into;
    every element of it is overwritten, so it needs no zeroing.
    -> DetectorInput.  In its targets the boxes are new tensors, the masks are new (G_i,nh_i,nw_i) uint8 tensors, not padded -- except
    that the masks of a frame whose size does not change are THE CALLER'S OWN TENSOR, returned as it is (do not write into it) -- and every
    other key holds the caller's own object.  A size with nh < 1 or nw < 1 is refused."""
    import torch
    parsed = _frames(frames, torch)
    B = len(parsed)
    table = pixel_table(image_mean, image_std)
    d = int(size_divisible)
    if d < 1 or d != size_divisible:
        raise ValueError(f'size_divisible must be a positive integer, got {size_divisible!r}')
    if not float(max_size) >= 1:
        raise ValueError(f'max_size must be at least 1, got {max_size!r}')
    mins = _min_sizes(min_size, B)
    tgt = None if targets is None else _check_targets(targets, parsed, torch)
    originals = [(h, w) for _, _, _, _, h, w in parsed]
    nets = [network_size(h, w, m, max_size) for (h, w), m in zip(originals, mins)]
    for i, ((h, w), (nh, nw)) in enumerate(zip(originals, nets)):
        if nh < 1 or nw < 1:
            raise ValueError(f'frame {i} of {h}x{w} would reach the network as {nh}x{nw} (min_size={mins[i]}, max_size={max_size})')
    Hp, Wp = padded_size(nets, d)
    n_planes = 0 if tgt is None else sum(int(m.shape[0]) for (_, m), o, s in zip(tgt, originals, nets) if m is not None and o != s)
    if B + n_planes > MAX_UNITS:
        raise ValueError(f'{B} frames and {n_planes} mask planes exceed the limit of {MAX_UNITS} per call')
    if Hp > MAX_ROWS or 3 * Hp * Wp >= 2 ** 31:
        raise ValueError(f'a batch of 3 x {Hp} x {Wp} images is too large: 3 Hp Wp must stay below 2^31 and Hp at or below {MAX_ROWS}')

    tensors = [p[0] for p in parsed]
    _lib.require_device(*tensors)
    device = tensors[0].device
    if any(t.device != device for t in tensors):
        raise ValueError('the frames live on one device')
    out = _lib.out_or_new(out, 'out', (B, 3, Hp, Wp), torch.float32, device, _empty)

    # one table: the 3 x 256 pixel values, the tap and nearest tables of every axis used, the mask planes' units; one descriptor per frame
    packer = TablePacker(table)

    # p00 alone holds the bits of the three fused operations at scale 1 unless a table entry is -0.0 (0 * p01 may be -0.0 and p00 + -0.0 is
    # p00 for every p00 but -0.0 + +0.0): such a table, which no positive std gives, takes the general path
    plain = not bool((np.signbit(table) & (table == 0)).any())
    items = np.zeros(B, ITEM_DTYPE)
    keep, units, new_targets = [], [], None
    for i, ((t, sc, sy, sx, h, w), (nh, nw)) in enumerate(zip(parsed, nets)):
        it = items[i]
        it['frame'], it['sc'], it['sy'], it['sx'] = t.data_ptr(), sc, sy, sx
        it['h'], it['w'], it['nh'], it['nw'] = h, w, nh, nw
        if plain and (nh, nw) == (h, w):
            it['flags'] = ONE_TAP
        else:
            (it['xb'], it['xn']), (it['yb'], it['yn']) = axis_offsets(packer, w, nw), axis_offsets(packer, h, nh)
    if tgt is not None:
        for i, (b, m) in enumerate(tgt):
            _lib.require_device(b, m)
            if b.device != device or (m is not None and m.device != device):
                raise ValueError(f'targets[{i}] must live on its frame\'s device {device}')
        total_boxes = sum(int(b.shape[0]) for b, _ in tgt)
        mask_at, mask_bytes = [], 0
        for (_, m), (h, w), (nh, nw) in zip(tgt, originals, nets):
            resized = m is not None and (h, w) != (nh, nw)
            mask_at.append(mask_bytes if resized else None)
            if resized:
                mask_bytes += -(-int(m.shape[0]) * nh * nw // 16) * 16     # every image's planes start at a multiple of 16 bytes
        boxes_out = _empty((total_boxes, 4), torch.float32, device)
        masks_out = _empty((mask_bytes,), torch.uint8, device)
        new_targets, row = [], 0
        for i, ((b, m), (h, w), (nh, nw), src) in enumerate(zip(tgt, originals, nets, targets)):
            it, G = items[i], int(b.shape[0])
            new = dict(src)
            new['boxes'] = boxes_out[row:row + G]
            if G:
                b = b.contiguous()
                keep.append(b)
                it['boxes'], it['boxes_out'], it['n_boxes'] = b.data_ptr(), new['boxes'].data_ptr(), G
                it['rw'], it['rh'] = box_ratios(h, w, nh, nw)
            row += G
            if mask_at[i] is not None:
                new['masks'] = masks_out[mask_at[i]:mask_at[i] + G * nh * nw].view(G, nh, nw)
                if G:
                    m = m.contiguous()
                    keep.append(m)
                    it['masks'], it['masks_out'], it['n_masks'] = m.data_ptr(), new['masks'].data_ptr(), G
                    units.extend((i, g) for g in range(G))   # the nearest tables of a resized frame are placed already
            new_targets.append(new)
    units_at = packer.append(np.asarray(units, np.int32))
    blob_d, items_p, tables_p, n_tables = packer.upload(items, device)
    with torch.cuda.device(device):
        _lib.check(_lib.lib().cosy_detector_input(items.ctypes.data, items_p, B, Hp, Wp, tables_p, n_tables, 0, units_at, len(units), _lib.ptr(out),
                                                 _lib.stream()))
    del keep
    return DetectorInput(out, nets, (Hp, Wp), originals, new_targets)


def _feature_list(backbone, images):
    import torch
    feats = backbone(images)
    if isinstance(feats, dict):                              # torchvision's backbones return an OrderedDict: its values in order
        feats = list(feats.values())
    elif torch.is_tensor(feats):
        feats = [feats]
    return list(feats)


def detections_from_frames(frames, backbone, rpn_head, box_head, mask_head, category_id_to_label, min_size=480, max_size=640,
                           image_mean=IMAGE_MEAN, image_std=IMAGE_STD, size_divisible=32, rpn_min_size=None, **filters):
    """Raw uint8 frames -> detections: detector_input, backbone(images) -> the list of feature maps (an OrderedDict's values in order),
    detector_rpn.detections_from_features.  min_size and max_size are the transform's; the RPN's own small-box threshold, which
    detections_from_features calls min_size, is rpn_min_size here (None: its default).  Everything in `filters` goes to
    detections_from_features unchanged."""
    from .detector_rpn import detections_from_features
    inp = detector_input(frames, None, min_size, max_size, image_mean, image_std, size_divisible)
    if rpn_min_size is not None:
        filters['min_size'] = rpn_min_size
    return detections_from_features(_feature_list(backbone, inp.images), rpn_head, box_head, mask_head, inp.net_sizes, inp.padded_size,
                                    inp.original_sizes, category_id_to_label, **filters)


def detector_losses_from_frames(frames, targets, backbone, rpn_head, box_head, mask_head, min_size=480, max_size=640, image_mean=IMAGE_MEAN,
                                image_std=IMAGE_STD, size_divisible=32, keys=None, generator=None, rpn_min_size=None, **options):
    """Raw uint8 frames and their targets (boxes, labels, masks at the frames' sizes) -> the reference's loss_dict: detector_input,
    backbone(images), detector_train.detector_losses.  min_size and max_size are the transform's; detector_losses' own min_size is
    rpn_min_size here (None: its default).  keys, generator and everything in `options` go to detector_losses unchanged."""
    from .detector_train import detector_losses
    inp = detector_input(frames, targets, min_size, max_size, image_mean, image_std, size_divisible)
    if rpn_min_size is not None:
        options['min_size'] = rpn_min_size
    return detector_losses(_feature_list(backbone, inp.images), rpn_head, box_head, mask_head, inp.targets, inp.net_sizes, inp.padded_size,
                           keys=keys, generator=generator, **options)


class _CallableModule(types.ModuleType):
    """`cosypose_amd.detector_input` names this module once it is imported and the function before: calling either is the function"""

    def __call__(self, *args, **kwargs):
        return detector_input(*args, **kwargs)

    __call__.__doc__ = detector_input.__doc__


sys.modules[__name__].__class__ = _CallableModule
