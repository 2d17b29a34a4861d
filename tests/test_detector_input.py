"""GPU tests of the detector's input side (cosypose_amd/detector_input.py, csrc/kernels_detin.hip) against the numpy
twin tests/detin_ref.py: BIT FOR BIT on the images (compared as uint32, so the padding's +0.0 and the sign of zero count), on the masks and
on the boxes; sizes equal.  The shapes are the smallest at which the kernel can still go wrong: the one-tap path next to the general one, a
width that is no multiple of the 4-column vector or of the padding, the floor's quirk, a 1 x 1 frame, mixed sizes in one launch, every
memory layout of a frame, reused output buffers between guards, the raw C ABI by hand, and the two chains on section 22's grid."""
import numpy as np
import pytest
import torch

import detin_ref as ref
from cosypose_amd import _lib, detections_from_features, detections_from_frames, detector_input, detector_losses_from_frames
from cosypose_amd import detector_input as di
from cosypose_amd import detector_train as dt

pytestmark = pytest.mark.gpu
f32 = np.float32
SENTINEL = 7
NAN_BITS = 0x7fc00123                                                            # a NaN no arithmetic produces

# (h, w, min_size, max_size) -> (nh, nw)
SINGLE = {(48, 64, 48, 64): (48, 64), (54, 72, 48, 64): (48, 64), (45, 60, 48, 64): (48, 64), (96, 128, 48, 64): (48, 64),
          (30, 100, 48, 64): (19, 64), (49, 70, 32, 64): (31, 45), (5, 7, 5, 7): (5, 7), (1, 1, 1, 1): (1, 1)}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def frame_of(h, w, seed=0):
    return np.random.RandomState(seed + 131 * h + w).randint(0, 256, (3, h, w)).astype(np.uint8)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def check(got, want, label=''):
    """a DetectorInput against the twin's dict: sizes equal, images bit-equal"""
    assert got.net_sizes == want['net_sizes'] and tuple(got.padded_size) == want['padded_size'] and got.original_sizes == want['original_sizes'], label
    images = host(got.images)
    assert images.dtype == f32 and images.shape == want['images'].shape, label
    bad = int((bits(images) != bits(want['images'])).sum())
    print(f'{label}: {bad} of {images.size} floats differ in their bits')
    assert bad == 0, label


def check_targets(got, want, sources):
    for b, (g, w, src) in enumerate(zip(got, want, sources)):
        assert set(g) == set(src)
        boxes = host(g['boxes'])
        assert boxes.dtype == f32 and boxes.shape == w['boxes'].shape and np.array_equal(bits(boxes), bits(w['boxes'])), b
        if 'masks' in src:
            masks = host(g['masks'])
            assert masks.dtype == np.uint8 and masks.shape == w['masks'].shape and np.array_equal(masks, w['masks']), b
        for key in src:
            if key not in ('boxes', 'masks'):
                assert g[key] is src[key], (b, key)


# ---- single frames and one mixed batch -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', list(SINGLE), ids=lambda c: f'{c[0]}x{c[1]}_at_{c[2]}_{c[3]}')
def test_single_frame_equals_the_twin(case):
    h, w, lo, hi = case
    f = frame_of(h, w)
    want = ref.transform([f], None, lo, hi)
    assert want['net_sizes'] == [SINGLE[case]]
    got = detector_input([dev(f)], min_size=lo, max_size=hi)
    assert got.targets is None and got.images.is_cuda
    check(got, want, f'{h}x{w} at {lo}/{hi}')


def mixed_frames():
    return [frame_of(54, 72), frame_of(30, 100), frame_of(49, 70), frame_of(5, 7)], [48, 15, 32, 5]       # 30 x 100 at 15: half its size


def test_mixed_batch_equals_the_twin():
    frames, mins = mixed_frames()
    want = ref.transform(frames, None, mins, 64)
    assert want['net_sizes'] == [(48, 64), (15, 50), (31, 45), (5, 7)] and want['padded_size'] == (64, 64)
    assert sum(nh < 64 and nw < 64 for nh, nw in want['net_sizes']) == 3                   # every image but one is smaller on both axes
    check(detector_input([dev(f) for f in frames], min_size=mins, max_size=64), want, 'four sizes, min_size per image')
    # one batch tensor, channels first and channels last
    same = np.stack([frame_of(45, 60, s) for s in range(3)])
    want = ref.transform(list(same), None, 48, 64)
    check(detector_input(dev(same), min_size=48, max_size=64), want, '(B,3,h,w)')
    check(detector_input(dev(same.transpose(0, 2, 3, 1)), min_size=48, max_size=64), want, '(B,h,w,3)')


def test_every_layout_of_a_frame_gives_the_same_bits():
    for (h, w, lo, hi) in ((48, 64, 48, 64), (49, 70, 32, 64), (45, 60, 48, 64)):         # the one-tap path and the general one
        f = frame_of(h, w, 3)
        want = ref.transform([f], None, lo, hi)
        hwc = dev(f.transpose(1, 2, 0))
        assert hwc.is_contiguous() and tuple(hwc.shape) == (h, w, 3)
        big = torch.randint(0, 256, (3, h + 5, w + 7), dtype=torch.uint8, device='cuda')
        big[:, 2:2 + h, 3:3 + w] = dev(f)
        big_hwc = torch.randint(0, 256, (h + 4, w + 6, 4), dtype=torch.uint8, device='cuda')
        big_hwc[1:1 + h, 5:5 + w, 1:4] = hwc
        layouts = {'CHW': dev(f), 'HWC': hwc, 'permute view of HWC': hwc.permute(2, 0, 1), 'slice of a larger CHW': big[:, 2:2 + h, 3:3 + w],
                   'slice of a larger HWC with 4 channels': big_hwc[1:1 + h, 5:5 + w, 1:4], 'every second column': dev(np.repeat(f, 2, axis=2))[:, :, ::2]}
        assert not layouts['permute view of HWC'].is_contiguous() and not layouts['slice of a larger CHW'].is_contiguous()
        for name, t in layouts.items():
            ptr = t.data_ptr()
            got = detector_input([t], min_size=lo, max_size=hi)
            assert t.data_ptr() == ptr
            check(got, want, f'{h}x{w} {name}')


def test_constant_frames_and_every_byte_value():
    for lo, hi, h, w in ((48, 64, 48, 64), (48, 64, 54, 72)):
        for value in (0, 255):
            f = np.full((3, h, w), value, np.uint8)
            check(detector_input([dev(f)], min_size=lo, max_size=hi), ref.transform([f], None, lo, hi), f'all {value}, {h}x{w}')
    ramp = np.broadcast_to(np.arange(256, dtype=np.uint8), (3, 6, 256)).copy()            # every byte value in every channel
    ramp[:, 1::2] = ramp[:, 1::2, ::-1]
    for lo, hi in ((6, 256), (5, 200), (9, 400)):
        want = ref.transform([ramp], None, lo, hi)
        check(detector_input([dev(ramp)], min_size=lo, max_size=hi), want, f'ramp at {lo}/{hi} -> {want["net_sizes"][0]}')
    table = ref.pixel_table()
    got = host(detector_input([dev(ramp)], min_size=6, max_size=256, size_divisible=1).images)[0]
    assert np.array_equal(bits(got[:, 0]), bits(table))                                    # the table itself, channel by channel


@pytest.mark.parametrize('mean,std', [((0.0, 0.0, 0.0), (1.0, 0.5, 2.0)), ((0.3, 0.6, 0.9), (0.1, 0.25, 0.7)), ((1.0, 0.0, 1.0), (-0.5, 1.0, 1.0))])
def test_other_means_and_stds(mean, std):
    frames, mins = [frame_of(48, 64, 1), frame_of(54, 72, 1)], [48, 48]
    frames[0][:, :4] = 0                                                                   # mean 0: p(0) = +0.0; std < 0: p may be -0.0
    frames[0][0, 4:8] = np.array([127, 128, 255, 0], np.uint8)[:, None]
    want = ref.transform(frames, None, mins, 64, mean, std)
    check(detector_input([dev(f) for f in frames], min_size=mins, max_size=64, image_mean=mean, image_std=std), want, f'mean {mean} std {std}')


@pytest.mark.parametrize('divisible', [1, 64])
def test_size_divisible(divisible):
    frames, mins = mixed_frames()
    frames, mins = frames[1:], mins[1:]                                                    # (15,50), (31,45), (5,7)
    want = ref.transform(frames, None, mins, 64, size_divisible=divisible)
    assert want['padded_size'] == {1: (31, 50), 64: (64, 64)}[divisible]
    check(detector_input([dev(f) for f in frames], min_size=mins, max_size=64, size_divisible=divisible), want, f'size_divisible={divisible}')
    f = frame_of(49, 70)                                                                   # rows of 45 floats: no 16-byte alignment
    want = ref.transform([f, f], None, 32, 64, size_divisible=1)
    assert want['padded_size'] == (31, 45)
    check(detector_input([dev(f), dev(f)], min_size=32, max_size=64, size_divisible=1), want, 'rows of 45 floats')


@pytest.mark.parametrize('guard', [64, 1])                                                # 16-byte aligned rows, and rows one float off
def test_reused_out_buffer_between_guards(guard):
    frames, mins = mixed_frames()
    want = ref.transform(frames, None, mins, 64)
    shape = want['images'].shape
    size = int(np.prod(shape))
    buf = torch.full((size + 2 * guard,), NAN_BITS, dtype=torch.int32, device='cuda').view(torch.float32)
    out = buf[guard:guard + size].view(shape)
    tensors = [dev(f) for f in frames]
    got = detector_input(tensors, min_size=mins, max_size=64, out=out)
    assert got.images.data_ptr() == out.data_ptr()
    check(got, want, f'out= with guards of {guard}')
    first = host(buf).view(np.uint32).copy()
    assert (first[:guard] == NAN_BITS).all() and (first[guard + size:] == NAN_BITS).all() and not (first[guard:guard + size] == NAN_BITS).any()
    out.fill_(-3.0)                                                                        # a used buffer: no zeroing is needed
    detector_input(tensors, min_size=mins, max_size=64, out=out)
    assert np.array_equal(host(buf).view(np.uint32), first)
    fresh = detector_input(tensors, min_size=mins, max_size=64)                            # the same without out=
    assert np.array_equal(bits(host(fresh.images)), bits(want['images']))
    with pytest.raises(ValueError, match='out must be'):
        detector_input(tensors, min_size=mins, max_size=64, out=out[:, :, :-1])


# ---- targets ---------------------------------------------------------------------------------------------------------------------------
FILL = 0xA5


class GuardedOutputs:
    """wraps detector_input._empty, where the wrapper allocates its outputs: each lies in a buffer filled with FILL, 64 elements of guard on
    either side.  untouched() says whether every byte of a buffer outside the given tensors still holds FILL."""

    def __init__(self, monkeypatch, guard=64):
        self.buffers = []

        def empty(shape, dtype, device):
            n, size = int(np.prod(shape)), torch.empty((), dtype=dtype).element_size()
            raw = torch.full(((n + 2 * guard) * size,), FILL, dtype=torch.uint8, device=device)
            self.buffers.append(raw)
            return raw[guard * size:(guard + n) * size].view(dtype).view(shape)
        monkeypatch.setattr(di, '_empty', empty)

    def untouched(self, raw, tensors):
        seen = host(raw).copy()
        outside = np.ones(seen.size, bool)
        for t in (t for t in tensors if t.numel()):
            start = t.data_ptr() - raw.data_ptr()
            assert 0 <= start and start + t.numel() * t.element_size() <= seen.size and t.is_contiguous()
            outside[start:start + t.numel() * t.element_size()] = False
        assert outside.sum() >= 128                                                         # the two guards at least
        return bool((seen[outside] == FILL).all()), int(outside.sum())


def check_guards(guards, got):
    """the wrapper's three buffers of one call (images, boxes, masks): nothing outside the tensors it handed out was written"""
    images, boxes, masks = guards.buffers[-3:]
    resized = [g['masks'] for g, net, orig in zip(got.targets, got.net_sizes, got.original_sizes) if 'masks' in g and net != orig]
    for name, raw, tensors in (('images', images, [got.images]), ('boxes', boxes, [g['boxes'] for g in got.targets]), ('masks', masks, resized)):
        ok, n = guards.untouched(raw, tensors)
        print(f'{name}: {n} bytes of guards and gaps, untouched: {ok}')
        assert ok, name


def test_targets_boxes_masks_and_passed_keys(monkeypatch):
    guards = GuardedOutputs(monkeypatch)
    rs = np.random.RandomState(8)
    frames = [frame_of(54, 72, 2), frame_of(48, 64, 2), frame_of(49, 70, 2), frame_of(30, 100, 2), frame_of(45, 60, 2), frame_of(96, 128, 2)]
    # G = 3, 65, 0 and 1 reach the mask path in one batch; the second frame keeps its size, the last has boxes and no masks
    mins, counts = [48, 48, 32, 48, 48, 48], [3, 2, 65, 0, 1, 2]
    targets_np, targets = [], []
    for f, G in zip(frames, counts):
        _, h, w = f.shape
        boxes = rs.uniform(-10, 110, (G, 4)).astype(f32)
        if G >= 3:
            boxes[0], boxes[1], boxes[2] = (5, 6, 5, 6), (-7.25, -3, -1, 12), (0, 0, w, h)      # zero area, negative, the whole frame
        masks = (rs.uniform(0, 1, (G, h, w)) < 0.5).astype(np.uint8) * rs.randint(1, 256, (G, 1, 1)).astype(np.uint8)
        targets_np.append(dict(boxes=boxes, masks=masks))
        targets.append(dict(boxes=dev(boxes), masks=dev(masks), labels=torch.arange(G), image_id=object()))
    del targets_np[5]['masks'], targets[5]['masks']                                        # masks are optional
    want = ref.transform(frames, targets_np, mins, 64)
    assert want['net_sizes'][1] == (48, 64) and all(n != o for k, (n, o) in enumerate(zip(want['net_sizes'], want['original_sizes'])) if k != 1)
    got = detector_input([dev(f) for f in frames], targets, min_size=mins, max_size=64)
    check(got, want, 'six frames with targets')
    check_targets(got.targets, want['targets'], targets)
    check_guards(guards, got)                                                              # 16-byte gaps between the images' planes included
    assert [int(g['masks'].shape[0]) for k, g in enumerate(got.targets) if k not in (1, 5)] == [3, 65, 0, 1]
    assert tuple(got.targets[4]['masks'].shape) == (1, 48, 64) and 'masks' not in got.targets[5]
    assert got.targets[1]['masks'] is targets[1]['masks']                                  # unchanged size: the caller's own tensor
    assert tuple(got.targets[3]['masks'].shape) == (0, 19, 64) and tuple(got.targets[3]['boxes'].shape) == (0, 4)
    assert all(g['masks'].is_contiguous() for g in got.targets if 'masks' in g) and all(g is not s for g, s in zip(got.targets, targets))
    again = detector_input([dev(f) for f in frames], targets, min_size=mins, max_size=64)
    check_targets(again.targets, want['targets'], targets)
    # non-contiguous boxes and masks are read as their values
    wide = dev(np.concatenate([targets_np[0]['boxes'], targets_np[0]['boxes']], 1))[:, :4]
    tall = dev(np.repeat(targets_np[0]['masks'], 2, axis=1))[:, ::2]
    assert not wide.is_contiguous() and not tall.is_contiguous()
    one = detector_input([dev(frames[0])], [dict(boxes=wide, masks=tall)], min_size=48, max_size=64)
    check_targets(one.targets, want['targets'][:1], [dict(boxes=wide, masks=tall)])


def test_masks_wider_than_a_tile(monkeypatch):
    """a tile is 8 rows of 128 columns: a mask of 600 columns takes five of them across, the last with 88 bytes, beside a narrow one whose
    rows end inside the first tile, in a batch padded to 32 x 608"""
    guards = GuardedOutputs(monkeypatch)
    rs = np.random.RandomState(11)
    frames = [frame_of(4, 300, 5), frame_of(12, 40, 5)]
    mins = [8, 24]                                                                         # 8 x 600 and 24 x 80
    counts = [23, 4]
    targets_np = [dict(boxes=rs.uniform(0, 50, (G, 4)).astype(f32), masks=rs.randint(0, 256, (G,) + f.shape[1:]).astype(np.uint8))
                  for G, f in zip(counts, frames)]
    want = ref.transform(frames, targets_np, mins, 600)
    assert want['net_sizes'] == [(8, 600), (24, 80)] and want['padded_size'] == (32, 608)
    targets = [dict(boxes=dev(t['boxes']), masks=dev(t['masks'])) for t in targets_np]
    got = detector_input([dev(f) for f in frames], targets, min_size=mins, max_size=600)
    check(got, want, 'wide masks')
    check_targets(got.targets, want['targets'], targets)
    check_guards(guards, got)


# ---- the raw C ABI by hand -------------------------------------------------------------------------------------------------------------
class Call:
    """a C entry point with a valid argument list by name; check() replaces some and wants -1 with untouched outputs"""

    def __init__(self, fn, outputs, **args):
        self.fn, self.outputs, self.args = fn, outputs, args

    def __call__(self, **kw):
        assert set(kw) <= set(self.args), set(kw) - set(self.args)
        return self.fn(*[kw.get(k, v) for k, v in self.args.items()])

    def untouched(self):
        return all(bool((t == SENTINEL).all()) for t in self.outputs)

    def check(self, name, bads, noops):
        for t in self.outputs:
            t.fill_(SENTINEL)
        assert self() == 0
        torch.cuda.synchronize()
        assert not self.untouched()                                             # the valid call does write
        wrong = []
        for label, bad in bads:
            for t in self.outputs:
                t.fill_(SENTINEL)
            rc = self(**bad)
            torch.cuda.synchronize()
            if rc != -1 or not self.untouched():
                wrong.append((label, rc))
        print(f'{name}: {len(bads)} violations, not refused with -1 and untouched outputs: {wrong}')
        assert not wrong
        for noop in noops:
            for t in self.outputs:
                t.fill_(SENTINEL)
            assert self(**noop) == 0, noop
            torch.cuda.synchronize()
            assert self.untouched(), noop


def by_hand(frame_d, masks_d, boxes_d, nh, nw, masks_out, boxes_out, table):
    """one item and its tables, the twin's, in the package's layout -> items (1,), tables, offset of the units"""
    from cosypose_amd._tables import TablePacker
    _, h, w = frame_d.shape
    G = int(masks_d.shape[0])
    packer = TablePacker(table)
    place = {key: packer.place(key, *ref.axis_ints(*key), align_ints=4) for key in ((w, nw), (h, nh))}
    units_at = packer.append(np.array([(0, g) for g in range(G)], np.int32))
    items = np.zeros(1, di.ITEM_DTYPE)
    it = items[0]
    it['frame'], it['sc'], it['sy'], it['sx'] = frame_d.data_ptr(), frame_d.stride(0), frame_d.stride(1), frame_d.stride(2)
    it['masks'], it['masks_out'], it['boxes'], it['boxes_out'] = masks_d.data_ptr(), masks_out.data_ptr(), boxes_d.data_ptr(), boxes_out.data_ptr()
    it['h'], it['w'], it['nh'], it['nw'], it['n_masks'], it['n_boxes'] = h, w, nh, nw, G, int(boxes_d.shape[0])
    (it['xb'], it['xn']), (it['yb'], it['yn']) = place[w, nw], place[h, nh]
    it['rw'], it['rh'] = f32(float(nw) / float(w)), f32(float(nh) / float(h))
    return items, np.concatenate(packer.parts), units_at


def test_c_abi_by_hand_and_its_refusals():
    lib = _lib.lib()
    h, w, nh, nw, Hp, Wp, G = 9, 14, 6, 10, 8, 12, 3
    rs = np.random.RandomState(17)
    f, m = rs.randint(0, 256, (3, h, w)).astype(np.uint8), rs.randint(0, 256, (G, h, w)).astype(np.uint8)
    b = rs.uniform(-5, 20, (2, 4)).astype(f32)
    table = ref.pixel_table()
    frame_d, masks_d, boxes_d = dev(f), dev(m), dev(b)
    guard = 32
    out_buf = torch.full((guard + 3 * Hp * Wp + guard,), SENTINEL, dtype=torch.float32, device='cuda')
    masks_buf = torch.full((guard + G * nh * nw + guard,), SENTINEL, dtype=torch.uint8, device='cuda')
    boxes_buf = torch.full((guard + 8 + guard,), SENTINEL, dtype=torch.float32, device='cuda')
    out, masks_out, boxes_out = out_buf[guard:-guard], masks_buf[guard:-guard], boxes_buf[guard:-guard]
    items, tables, units_at = by_hand(frame_d, masks_d, boxes_d, nh, nw, masks_out, boxes_out, table)
    n_tables = int(tables.size)

    def upload(items):
        blob = np.concatenate([items.view(np.uint8).reshape(-1), tables.view(np.uint8)])
        blob_d = dev(blob)
        assert blob_d.data_ptr() % 16 == 0
        return blob_d

    def variant(**changes):
        """the call's arguments for a changed copy of the item (host and device copies alike); the buffers stay alive in `kept`"""
        changed = items.copy()
        for key, value in changes.items():
            changed[key] = value
        blob_d = upload(changed)
        kept.append((changed, blob_d))
        return dict(items_host=changed.ctypes.data, items=blob_d.data_ptr(), tables=blob_d.data_ptr() + changed.nbytes)

    kept = []
    good = variant()
    call = Call(lib.cosy_detector_input, [out_buf, masks_buf, boxes_buf], n=1, Hp=Hp, Wp=Wp, n_tables=n_tables, lut=0, units=units_at, n_units=G,
                out_images=out.data_ptr(), stream=_lib.stream(), **good)
    call.args = {k: call.args[k] for k in ('items_host', 'items', 'n', 'Hp', 'Wp', 'tables', 'n_tables', 'lut', 'units', 'n_units', 'out_images', 'stream')}
    bads = [('null frame', variant(frame=0)), ('w = 0', variant(w=0)), ('h = -1', variant(h=-1)), ('nh = 0', variant(nh=0)),
            ('nw > Wp', variant(nw=Wp + 1)), ('xb outside the blob', variant(xb=n_tables - 4)), ('yb negative', variant(yb=-4)),
            ('xb misaligned', variant(xb=int(items['xb'][0]) + 2)), ('yn outside the blob', variant(yn=n_tables - nh + 1)),
            ('null masks', variant(masks=0)), ('null masks_out', variant(masks_out=0)), ('null boxes_out', variant(boxes_out=0)),
            ('negative stride', variant(sy=-1)), ('negative count', variant(n_masks=-1)),
            ('n = -1', dict(n=-1)), ('Hp = 0', dict(Hp=0)), ('Wp = 0', dict(Wp=0)), ('lut = -1', dict(lut=-1)), ('lut past the tables', dict(lut=n_tables - 767)),
            ('units past the tables', dict(units=n_tables - 2 * G + 1)), ('n_units = -1', dict(n_units=-1)), ('too many units', dict(n_units=65535)),
            ('null items_host', dict(items_host=None)), ('null items', dict(items=None)), ('null tables', dict(tables=None)),
            ('null out_images', dict(out_images=None)), ('tables off 16 bytes', dict(tables=good['tables'] + 4)),
            ('out_images off 4 bytes', dict(out_images=out.data_ptr() + 2))]
    noops = [dict(n=0), dict(n=0, items_host=None, items=None, tables=None, out_images=None)]
    call.check('cosy_detector_input', bads, noops)
    # the valid call by hand: the twin's bits between untouched guards, in all three outputs
    for t in (out_buf, masks_buf, boxes_buf):
        t.fill_(SENTINEL)
    assert call() == 0
    want = np.zeros((3, Hp, Wp), f32)
    want[:, :nh, :nw] = ref.image(f, nh, nw, table)
    got, got_m, got_b = host(out_buf), host(masks_buf), host(boxes_buf)
    assert np.array_equal(bits(got[guard:-guard]), bits(want.reshape(-1)))
    assert np.array_equal(got_m[guard:-guard].reshape(G, nh, nw), ref.masks(m, nh, nw))
    assert np.array_equal(bits(got_b[guard:-guard]), bits(ref.boxes(b, h, w, nh, nw).reshape(-1)))
    for g in (got, got_m, got_b):
        assert (g[:guard] == SENTINEL).all() and (g[-guard:] == SENTINEL).all()
    # the DEVICE copy alone is wrong (the host copy is the good one): the kernel skips the item, and a unit without an item or a plane
    for label, changes in (('null frame', dict(frame=0)), ('w = 0', dict(w=0)), ('xb outside the blob', dict(xb=n_tables - 4))):
        for t in (out_buf, masks_buf, boxes_buf):
            t.fill_(SENTINEL)
        device_only = variant(**changes)
        assert call(items=device_only['items'], tables=device_only['tables']) == 0
        torch.cuda.synchronize()
        assert call.untouched(), label
    for t in (out_buf, masks_buf, boxes_buf):
        t.fill_(SENTINEL)
    wrong_units = tables.copy()
    wrong_units[units_at:units_at + 4] = (1, 0, 0, G)                                      # an item and a plane that do not exist; (0, 2) stays
    blob_d = dev(np.concatenate([items.view(np.uint8).reshape(-1), wrong_units.view(np.uint8)]))
    assert call(items=blob_d.data_ptr(), tables=blob_d.data_ptr() + items.nbytes) == 0
    got_m = host(masks_buf)[guard:-guard].reshape(G, nh, nw)
    assert (got_m[:2] == SENTINEL).all() and np.array_equal(got_m[2], ref.masks(m, nh, nw)[2])
    assert np.array_equal(bits(host(out_buf)[guard:-guard]), bits(want.reshape(-1)))


# ---- the chains, on section 22's grid ----------------------------------------------------------------------------------------------------
GRID, A = [(5, 7), (3, 4), (1, 2)], 3
SIZES, RATIOS = ((32,), (64,), (128,)), (0.5, 1.0, 2.0)
PAD, NETS = (40, 56), [(37, 53), (40, 50)]
CHAIN = dict(min_size=[37, 40], max_size=56, size_divisible=8)                            # 74 x 106 -> 37 x 53, 20 x 25 -> 40 x 50
NAMES = {1: 'obj_000001', 2: 'obj_000002'}


def chain_frames(sizes=(((74, 106), 12), ((20, 25), 4)), seed=4):
    """blocks of colour, so that the pooled feature maps differ from cell to cell"""
    rs = np.random.RandomState(seed)
    out = []
    for (h, w), cell in sizes:
        coarse = rs.randint(0, 256, (3, -(-h // cell), -(-w // cell)))
        out.append((np.kron(coarse, np.ones((cell, cell)))[:, :h, :w] * rs.uniform(0.8, 1.0, (3, h, w))).astype(np.uint8))
    return out


class Backbone:
    """strided average pools to the grid's sizes and a fixed lift from 3 to C channels, in torch"""

    def __init__(self, C=8, seed=2):
        g = torch.Generator().manual_seed(seed)
        self.lift = [(torch.randn((C, 3), generator=g) * 1.5).cuda() for _ in GRID]
        self.grads = False

    def __call__(self, images):
        assert tuple(images.shape[2:]) == PAD
        out = []
        for (H, W), lift in zip(GRID, self.lift):
            pooled = torch.nn.functional.adaptive_avg_pool2d(images, (H, W))
            out.append(torch.einsum('kc,bchw->bkhw', lift, pooled).contiguous().requires_grad_(self.grads))
        return dict(zip('012', out))                                                       # a dict, as torchvision's backbones return


class Heads:
    """the tiny heads of tests/test_detector_rpn.py and tests/test_detector_train.py: the RPN's size deltas are zero, the box and mask heads run in
    float64 and round once"""

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


def test_detections_from_frames_equal_the_chain_fed_by_the_twin():
    frames = chain_frames((((74, 106), 12), ((74, 106), 9)))                               # masks need all frames of one size
    chain = dict(CHAIN, min_size=[37, 27])
    twin = ref.transform(frames, None, chain['min_size'], chain['max_size'], size_divisible=chain['size_divisible'])
    assert twin['net_sizes'][0] == NETS[0] and twin['net_sizes'][1][0] in (26, 27) and twin['padded_size'] == PAD
    heads, backbone = Heads(), Backbone()
    options = dict(sizes=SIZES, pre_nms_top_n=64, post_nms_top_n=20, detections_per_img=100, output_masks=True, n_roi_levels=2, score_thresh=0.0)
    with torch.no_grad():
        got = detections_from_frames([dev(f) for f in frames], backbone, heads.rpn, heads.box, heads.mask_head, NAMES, **chain, **options)
        feats = list(backbone(dev(twin['images'])).values())
        want = detections_from_features(feats, heads.rpn, heads.box, heads.mask_head, twin['net_sizes'], twin['padded_size'], twin['original_sizes'],
                                        NAMES, **options)
    print(f'{len(want.infos)} detections in images {sorted(set(want.infos["batch_im_id"].tolist()))}')
    assert len(want.infos) >= 2
    assert got.infos['batch_im_id'].tolist() == want.infos['batch_im_id'].tolist() and got.infos['label'].tolist() == want.infos['label'].tolist()
    assert np.array_equal(bits(got.infos['score'].values), bits(want.infos['score'].values))
    assert np.array_equal(bits(host(got.bboxes)), bits(host(want.bboxes)))
    assert got.masks.shape == want.masks.shape and tuple(got.masks.shape[1:]) == (74, 106) and bool((got.masks == want.masks).all())


def test_detector_losses_from_frames_equal_the_chain_fed_by_the_twin():
    frames = chain_frames()
    rs = np.random.RandomState(6)
    gt = [np.array([[16, 0, 80, 64], [40, 20, 100, 72], [0, 0, 40, 36]], f32), np.array([[1, 1.5, 15, 15], [12, 2, 25, 17]], f32)]
    labels = [[1, 2, 1], [2, 1]]
    masks = [(rs.uniform(0, 1, (len(g),) + f.shape[1:]) < 0.5).astype(np.uint8) for g, f in zip(gt, frames)]
    n_anchors = sum(H * W for H, W in GRID) * A
    keys = dict(rpn=rs.randint(0, 2 ** 31 - 1, (2, n_anchors)).astype(np.int32), roi=rs.randint(0, 2 ** 31 - 1, (2, 20 + 3)).astype(np.int32))
    targets_np = [dict(boxes=g, masks=m) for g, m in zip(gt, masks)]
    twin = ref.transform(frames, targets_np, CHAIN['min_size'], CHAIN['max_size'], size_divisible=CHAIN['size_divisible'])
    options = dict(n_roi_levels=2, sizes=SIZES, aspect_ratios=RATIOS, pre_nms_top_n=64, post_nms_top_n=20)

    def run(from_frames):
        heads, backbone = Heads(), Backbone()
        backbone.grads = True
        targets = [dict(boxes=dev(g), labels=dev(np.asarray(l, np.int64)), masks=dev(m)) for g, l, m in zip(gt, labels, masks)]
        device_keys = {k: dev(v) for k, v in keys.items()}
        if from_frames:
            losses = detector_losses_from_frames([dev(f) for f in frames], targets, backbone, heads.rpn, heads.box, heads.mask_head, keys=device_keys,
                                                 **CHAIN, **options)
        else:
            fed = [dict(boxes=dev(t['boxes']), labels=s['labels'], masks=dev(t['masks'])) for t, s in zip(twin['targets'], targets)]
            feats = list(backbone(dev(twin['images'])).values())
            losses = dt.detector_losses(feats, heads.rpn, heads.box, heads.mask_head, fed, twin['net_sizes'], twin['padded_size'], keys=device_keys,
                                        **options)
        sum(losses.values()).backward()
        return losses, heads

    got, heads = run(True)
    want, _ = run(False)
    assert tuple(got) == dt.LOSS_KEYS
    for name in dt.LOSS_KEYS:
        a, b = host(got[name]).reshape(1), host(want[name]).reshape(1)
        print(f'{name}: {a[0]!r} from frames, {b[0]!r} fed by the twin')
        assert np.isfinite(a).all() and np.array_equal(bits(a), bits(b)), name
    grad = heads.fc.weight.grad
    assert grad is not None and bool(torch.isfinite(grad).all()) and bool(grad.any())
    grad = heads.conv.weight.grad
    assert grad is not None and bool(torch.isfinite(grad).all()) and bool(grad.any())
