"""numpy restatement of DESIGN.md section 25: the detector's input side (torchvision 0.4.2's GeneralizedRCNNTransform on torch 1.3) for uint8
frames -- the size rule in Python doubles, the 3 x 256 pixel table, float32 bilinear interpolation with half-pixel centres written as three
fused multiply-adds, +0.0 padding into one batch, boxes times a float32 ratio, masks through nearest.  Independent of the package: nothing
here imports cosypose_amd.  The taps of an axis, the nearest indices and the emulation of fmaf (which raises where float64 cannot promise
one rounding) are section 18's and come from frames_ref.

Also the float64 value of every pixel and the per-pixel bound that separates this twin from F.interpolate of the installed torch
(`bilinear_bound`): the two routes share the real bilinear form but neither the order of its roundings nor the last bits of its weights.
"""
import math

import numpy as np

import frames_ref

F32 = np.float32
U = 2.0 ** -24                                 # unit roundoff of float32
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
ROUNDINGS = 15                                 # see bilinear_bound
COORD_ULPS = 2                                 # see bilinear_bound


def network_size(h, w, min_size, max_size):
    s = float(min_size) / float(min(h, w))
    if float(max(h, w)) * s > max_size:
        s = float(max_size) / float(max(h, w))
    return int(math.floor(float(h) * s)), int(math.floor(float(w) * s))


def padded_size(net_sizes, size_divisible=32):
    return tuple(int(math.ceil(float(max(s[k] for s in net_sizes)) / size_divisible) * size_divisible) for k in (0, 1))


def pixel_table(mean=MEAN, std=STD):
    """(3,256) float32: ((float32(u) / 255f) - mean_c) / std_c"""
    u = np.arange(256, dtype=F32)[None]
    m, s = np.asarray(mean, F32)[:, None], np.asarray(std, F32)[:, None]
    p = ((u / F32(255)).astype(F32) - m).astype(F32) / s
    assert p.dtype == F32 and p.shape == (3, 256)
    return p


def pixels(frame, table):
    """(3,h,w) uint8 -> (3,h,w) float32 through the table"""
    return np.stack([table[c][frame[c]] for c in range(3)])


def image(frame, nh, nw, table):
    """(3,h,w) uint8 -> (3,nh,nw) float32: the general path, whatever the sizes"""
    return frames_ref.two_tap(pixels(frame, table), nh, nw)


def image_float64(frame, nh, nw, table):
    """the same bilinear form with the twin's float32 weights and table, every product and sum in float64"""
    return frames_ref.two_tap_float64(pixels(frame, table), nh, nw)


def _coordinate_slack(n_in, n_out):
    """per output index: COORD_ULPS float32 ulps of the largest intermediate of the source coordinate, scale * (i + 0.5)"""
    scale = F32(n_in) / F32(n_out)
    x = (scale * (np.arange(n_out, dtype=F32) + F32(0.5))).astype(F32)
    return COORD_ULPS * np.spacing(x).astype(np.float64)


def _step(p, axis, i0):
    """(3,.,.) float64: the largest |difference| between neighbouring samples of p along `axis` among the three pairs around tap i0 (the tap's
    own pair and the one on either side: a coordinate that moves across an integer changes the pair)"""
    n = p.shape[axis]
    d = np.abs(np.diff(p, axis=axis))                                          # d[k] = |p[k+1] - p[k]|, n - 1 of them
    if n == 1:
        return np.zeros_like(np.take(p, i0, axis=axis))
    best = None
    for k in (-1, 0, 1):
        t = np.take(d, np.clip(i0 + k, 0, n - 2), axis=axis)
        best = t if best is None else np.maximum(best, t)
    return best


def bilinear_bound(frame, nh, nw, table):
    """(3,nh,nw) float64: how far F.interpolate(size=(nh, nw), mode='bilinear', align_corners=False) of a correct float32 implementation may
    lie from image().  Two parts.
    Roundings: either side evaluates v = ly0 (lx0 p00 + lx1 p01) + ly1 (lx0 p10 + lx1 p11) as three interpolations a = l0 p + l1 q.  One
    interpolation rounds its products by at most U (l0 |p| + l1 |q|) <= U M' together and its sum by U M', with M' = M (1 + 2 U) (the
    weights of an axis are l1 and fl(1 - l1), they sum to at most 1 + U): 2 U M', fused or not.  The two horizontal ones enter v with the
    weights ly0 + ly1, so a side is at most 4 U M' from the real form of its own weights, both sides 8; fl(1 - l1) is U / 2 from 1 - l1 and
    moves v by U M / 2 per axis and side, 2 more.  That is 10; the bound holds ROUNDINGS = 15 roundings of U M', the count of single
    operations (9 not fused, 6 fused), which is the looser of the two and the one DESIGN.md states.
    Weights: the source coordinate is fl(fl(scale (i + 0.5)) - 0.5) here, two roundings of values <= x = scale (i + 0.5), so at most one
    ulp32(x) from the real value; another correct evaluation (a fused multiply-add, another order) lies within one ulp32(x) too.  The
    coordinates differ by at most COORD_ULPS = 2 ulp32(x), and v is piecewise linear in each coordinate with slope |p_b - p_a| between two
    neighbouring samples: the x coordinate moves v by at most slack_x max |step along x| over the two rows, the y coordinate by slack_y
    max |step along y| over the two columns, the steps taken over the tap's pair and the pair on either side."""
    _, h, w = frame.shape
    p = pixels(frame, table).astype(np.float64)
    M = float(np.abs(table).max())
    y0, y1, _, _ = frames_ref.axis(h, nh)
    x0, x1, _, _ = frames_ref.axis(w, nw)
    sx = _step(p, 2, x0)                                                       # (3,h,nw)
    step_x = np.maximum(sx[:, y0], sx[:, y1])                                  # (3,nh,nw)
    sy = _step(p, 1, y0)                                                       # (3,nh,w)
    step_y = np.maximum(sy[:, :, x0], sy[:, :, x1])
    rounding = ROUNDINGS * U * M * (1 + 2 * U)
    weights = _coordinate_slack(w, nw)[None, None, :] * step_x + _coordinate_slack(h, nh)[None, :, None] * step_y
    return rounding + weights, rounding, weights


def boxes(b, h, w, nh, nw):
    """(G,4) float32 xyxy: x * rw, y * rh, the ratios double quotients rounded once to float32"""
    rw, rh = F32(float(nw) / float(w)), F32(float(nh) / float(h))
    out = np.asarray(b, F32).reshape(-1, 4) * np.array([rw, rh, rw, rh], F32)
    assert out.dtype == F32
    return out


def masks(m, nh, nw):
    """(G,h,w) uint8 -> (G,nh,nw) through nearest"""
    _, h, w = m.shape
    return np.ascontiguousarray(m[:, frames_ref.nearest_index(h, nh)][:, :, frames_ref.nearest_index(w, nw)])


def axis_ints(n_in, n_out):
    """the tables of one axis as the C ABI reads them: taps (n_out,4) int32 = i0, i1, bits of l0, bits of l1; nearest (n_out,) int32"""
    i0, i1, l0, l1 = frames_ref.axis(n_in, n_out)
    taps = np.stack([i0.astype(np.int32), i1.astype(np.int32), l0.view(np.int32), l1.view(np.int32)], 1)
    return np.ascontiguousarray(taps), frames_ref.nearest_index(n_in, n_out).astype(np.int32)


def transform(frames, targets=None, min_size=480, max_size=640, mean=MEAN, std=STD, size_divisible=32):
    """frames: list of (3,h_i,w_i) uint8 arrays; targets: None or list of dicts with boxes (G,4) and optionally masks (G,h,w); min_size an int
    or one per image -> dict(images (B,3,Hp,Wp) float32, net_sizes, padded_size, original_sizes, targets)"""
    B = len(frames)
    mins = list(min_size) if isinstance(min_size, (list, tuple)) else [min_size] * B
    table = pixel_table(mean, std)
    originals = [tuple(int(v) for v in f.shape[1:]) for f in frames]
    nets = [network_size(h, w, m, max_size) for (h, w), m in zip(originals, mins)]
    Hp, Wp = padded_size(nets, size_divisible)
    images = np.zeros((B, 3, Hp, Wp), F32)                                     # +0.0
    for i, (f, (nh, nw)) in enumerate(zip(frames, nets)):
        images[i, :, :nh, :nw] = image(f, nh, nw, table)
    out_targets = None
    if targets is not None:
        out_targets = []
        for t, (h, w), (nh, nw) in zip(targets, originals, nets):
            new = dict(t)
            new['boxes'] = boxes(t['boxes'], h, w, nh, nw)
            if t.get('masks') is not None:
                new['masks'] = t['masks'] if (h, w) == (nh, nw) else masks(t['masks'], nh, nw)
            out_targets.append(new)
    return dict(images=images, net_sizes=nets, padded_size=(Hp, Wp), original_sizes=originals, targets=out_targets)
