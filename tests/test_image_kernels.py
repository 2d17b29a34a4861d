"""The image kernels over the full byte range and at the edges of their tiles: the augmentations (csrc/kernels_aug.hip, DESIGN.md section
14), Pillow's resize (csrc/kernels_resize.hip, section 17) and the frames' own resize (csrc/kernels_frames.hip, section 18), each
against its numpy twin (aug_ref, resize_ref, frames_ref) -- every comparison is np.array_equal on uint8, there is no tolerance anywhere
in this file.  The inputs come from tests/image_edge_case.py; test_image_kernels_host.py proves on the twins alone that they reach what
they are for (every byte value after the blur, both clip branches of blend(), exact ties of Contrast's mean, the extremes of the bicubic
accumulator, sums that the fused multiply-add emulation can round).

A  augment_batch / cosy_augment_batch
   A1 block images whose block centres survive the blur: single stages over all 256 values, the full chain on 4096 colours, constants
   A2 sizes at the multiples and halo-wide remainders of the row tiles (8x128, halo 9) and column tiles (64x64, halo 10 rows, 1 column),
      with a frame that is lit only on the seams
   A3 Contrast's mean: exact ties, the largest sums, means 0, 1, 254 and 255, half-and-half frames of whole tiles
   A4 the C entry point's refusals
B  resize_images
   B1 lines that follow the signs of the taps: the int32 accumulator at its extremes, the arithmetic shift and both clips
   B2 constants stay constant
   B3 output widths and heights around the 4-row x 256-byte tile, one-pixel axes, 8001 taps, `out` at any byte offset
C  resize_frames / cosy_resize_frames_u8
   C1 every byte value, a 0/255 checkerboard and a ramp, masks with every id
   C2 outputs around the 8-row x 128-byte tile, `out` and `out_masks` at odd byte offsets
   C3 descriptors the kernel must skip and calls the entry point must refuse, by hand
Each test prints its mismatch counts before it asserts."""
import numpy as np
import pytest
import torch

import aug_ref
import frames_ref
import image_edge_case as case
import resize_ref

pytestmark = pytest.mark.gpu

SENTINEL = 7


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()                                 # a copy: the builders hand out read-only arrays


def augment(images, recs, masks=None, backgrounds=None):
    from cosypose_amd.augmentations import augment_batch
    with_bg = backgrounds is not None
    return augment_batch(dev(images), recs, masks=dev(masks) if with_bg else None, backgrounds=dev(backgrounds) if with_bg else None).cpu().numpy()


def report(label, got, want):
    per = [int((g != w).sum()) for g, w in zip(got, want)]
    print(f'{label}: {sum(per)} of {want.size} bytes differ; images that differ: {[(i, n) for i, n in enumerate(per) if n][:12]}')
    return sum(per)


def view_at(offset, shape, slack=8):
    """a contiguous uint8 view of `shape` at byte `offset` of a sentinel-filled device buffer -> (buffer, view)"""
    size = int(np.prod(shape))
    buf = torch.full((size + slack,), SENTINEL, dtype=torch.uint8, device='cuda')
    view = buf[offset:offset + size].view(shape)
    assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + offset
    return buf, view


def untouched_around(buf, offset, size):
    host = buf.cpu().numpy()
    return bool((host[:offset] == SENTINEL).all() and (host[offset + size:] == SENTINEL).all())


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
        for bad in bads:
            for t in self.outputs:
                t.fill_(SENTINEL)
            rc = self(**bad)
            torch.cuda.synchronize()
            if rc != -1 or not self.untouched():
                wrong.append((bad, rc))
        print(f'{name}: {len(bads)} violations, not refused with -1 and untouched outputs: {wrong}')
        assert not wrong
        for noop in noops:
            for t in self.outputs:
                t.fill_(SENTINEL)
            assert self(**noop) == 0, noop
            torch.cuda.synchronize()
            assert self.untouched(), noop


# ================================================================ A: augmentations
def test_aug_single_stages_over_every_byte_value():
    """A1: one record per (stage, factor) on values256, whose blurred channels hold all 256 values with steep steps between them"""
    image, _ = case.values256()
    labels, recs = zip(*case.single_stage_records())
    images = np.broadcast_to(image, (len(recs),) + image.shape)
    want = aug_ref.augment(images, recs)
    got = augment(images, list(recs))
    per = {label: int((g != w).sum()) for label, g, w in zip(labels, got, want)}
    print(f'values256, {len(recs)} records: {sum(per.values())} of {want.size} bytes differ; records that differ: { {k: v for k, v in per.items() if v} }')
    assert all(len(np.unique(want[labels.index(f'{name}=1.0')][c])) == 256 for name, _ in case.SINGLE_FACTORS for c in range(3))
    assert np.array_equal(got, want)


def test_aug_full_chain_on_4096_colours():
    """A1: all stages on, k = 1, 2, 3, on every combination of 16 levels per channel"""
    image, _ = case.colours4096()
    recs = case.full_chain_records()
    images = np.broadcast_to(image, (len(recs),) + image.shape)
    want = np.stack([aug_ref.augment_one(case.hwc(image), r).transpose(2, 0, 1) for r in recs])
    got = augment(images, recs)
    bad = report('colours4096, full chain', got, want)
    assert bad == 0 and np.array_equal(got, want)


@pytest.mark.parametrize('hw', ((3, 3), (20, 140)), ids=lambda hw: f'{hw[0]}x{hw[1]}')
def test_aug_a_constant_frame_comes_back_unchanged(hw):
    """A1: 256 constant frames in one call; the blur alone must return them, and with sharpness 2 SMOOTH's float32 sum and truncating
    cast must do what the twin does"""
    images, plain, sharp = case.constant_frames(*hw)
    got = augment(images, plain)
    changed = [v for v in range(256) if (got[v] != v).any()]
    print(f'{hw} blur only: {int((got != images).sum())} of {got.size} bytes changed; constants that changed: {changed}')
    assert np.array_equal(got, images)
    want = aug_ref.augment(images, sharp)
    got = augment(images, sharp)
    bad = report(f'{hw} sharpness 2.0', got, want)
    assert bad == 0 and np.array_equal(got, want)


@pytest.mark.parametrize('hw', case.AUG_EDGE_SIZES, ids=lambda hw: f'{hw[0]}x{hw[1]}')
def test_aug_tile_edges(hw):
    """A2: 0/255 noise and the frame lit only on the tile seams, k = 3 with sharpness and k = 1 alone, half of them pasted"""
    images, masks, backgrounds, recs = case.aug_edge_batch(*hw)
    want = aug_ref.augment(images, recs, masks, backgrounds)
    got = augment(images, recs, masks, backgrounds)
    bad = report(f'{hw}', got, want)
    if bad:
        ys, xs = np.nonzero((got != want).any(axis=(0, 1)))
        print(f'rows {sorted(set(ys.tolist()))[:20]} columns {sorted(set(xs.tolist()))[:20]}')
    assert np.array_equal(got, want)


def test_aug_contrast_mean_ties_and_range():
    """A3: frames whose mean of L is exactly x.5, and frames whose mean is 0, 1, 254 and 255; a mean that is off by one moves
    deg (1 - f) by 0.8 of a level at factor 0.2"""
    bad = {}
    ties = case.tie_frames()
    assert len(ties) >= 3
    frames = [(f'tie {im.shape[1]}x{im.shape[2]} mean {mean}', im) for im, mean in ties]
    frames += [(f'mean {mean}', im) for mean, im in sorted(case.mean_range_frames().items())]
    assert len(frames) >= 7
    recs = [case.rec(1, contrast=f) for f in case.CONTRAST_FACTORS]
    for label, im in frames:
        images = np.broadcast_to(im, (len(recs),) + im.shape)
        want = aug_ref.augment(images, recs)
        got = augment(images, recs)
        bad[label] = int((got != want).sum())
        print(f'{label}: {bad[label]} of {want.size} bytes differ; contrast 0.2 gives {got[0, 0].reshape(-1)[:6].tolist()}, the twin {want[0, 0].reshape(-1)[:6].tolist()}')
    assert not any(bad.values()), bad


def test_aug_contrast_largest_sums_and_half_frames():
    """A3: all 0 and all 255 at 130x259 (the largest sum of L, added by 15 workgroups), and half-0 / half-255 frames of whole tiles"""
    h, w = 130, 259
    images = np.stack([np.full((3, h, w), v, np.uint8) for v in (0, 0, 255, 255)])
    recs = [case.rec(1 + i % 3, contrast=f) for i, f in enumerate((0.2, 50.0, 0.2, 50.0))]
    want = aug_ref.augment(images, recs)
    got = augment(images, recs)
    bad = report(f'constants 0 and 255 at {h}x{w}', got, want)
    assert bad == 0 and np.array_equal(got, images)
    for hh, ww in case.HALF_SIZES:
        images = np.stack([case.half_frame(hh, ww, vertical) for vertical in (False, True) for _ in case.CONTRAST_FACTORS])
        recs = [case.rec(1, contrast=f) for _ in (False, True) for f in case.CONTRAST_FACTORS]
        want = aug_ref.augment(images, recs)
        got = augment(images, recs)
        bad += report(f'half frames {hh}x{ww}', got, want)
    assert bad == 0


def test_aug_c_abi_refusals():
    """A4: cosy_augment_batch by hand: a refused call returns -1 and leaves `out` untouched"""
    from cosypose_amd import _lib
    from cosypose_amd.augmentations import pack_params
    lib = _lib.lib()
    B, H, W, n_bg = 2, 5, 7, 2
    rs = np.random.RandomState(4)
    images, masks = dev(rs.randint(0, 256, (B, 3, H, W)).astype(np.uint8)), dev((rs.rand(B, H, W) < 0.5).astype(np.uint8))
    backgrounds = dev(rs.randint(0, 256, (n_bg, 3, H, W)).astype(np.uint8))
    params = dev(pack_params([case.rec(2, bg=1, sharpness=2.0, contrast=1.5), case.rec(1, bg=0, gray=True)]).view(np.int32).reshape(B, 8))
    out = torch.full((B, 3, H, W), SENTINEL, dtype=torch.uint8, device='cuda')
    need = lib.cosy_augment_workspace_bytes(B, H, W)
    assert need > 0 and need % 16 == 0
    ws = torch.zeros(need + 16, dtype=torch.uint8, device='cuda')
    assert ws.data_ptr() % 16 == 0
    call = Call(lib.cosy_augment_batch, [out], images=images.data_ptr(), masks=masks.data_ptr(), backgrounds=backgrounds.data_ptr(), n_bg=n_bg,
                params=params.data_ptr(), B=B, H=H, W=W, out=out.data_ptr(), workspace=ws.data_ptr(), workspace_bytes=need, stream=_lib.stream())
    bads = [dict(B=-1), dict(H=0), dict(W=0), dict(n_bg=-1), dict(images=None), dict(params=None), dict(out=None), dict(workspace=None),
            dict(masks=None), dict(backgrounds=None), dict(workspace_bytes=need - 1), dict(workspace=ws.data_ptr() + 8),
            dict(B=65536), dict(H=-3), dict(W=-1)]
    noops = [dict(B=0, images=None, masks=None, backgrounds=None, n_bg=0, params=None, out=None, workspace=None, workspace_bytes=0)]
    call.check('cosy_augment_batch', bads, noops)
    assert lib.cosy_augment_workspace_bytes(0, H, W) == 0 and lib.cosy_augment_workspace_bytes(B, 0, W) == 0
    # the valid call gives the twin's bytes, from the workspace of exactly the size asked for
    out.fill_(SENTINEL)
    assert call() == 0
    recs = [case.rec(2, bg=1, sharpness=2.0, contrast=1.5), case.rec(1, bg=0, gray=True)]
    want = aug_ref.augment(images.cpu().numpy(), recs, masks.cpu().numpy(), backgrounds.cpu().numpy())
    assert report('cosy_augment_batch by hand', out.cpu().numpy(), want) == 0


# ================================================================ B: Pillow resize
def resize(images, size, resample, out=None):
    from cosypose_amd.resize import resize_images
    return resize_images(dev(images), size, resample, out=out).cpu().numpy()


@pytest.mark.parametrize('resample', case.FILTERS)
def test_resize_accumulator_extremes(resample):
    """B1: source lines that follow the signs of the taps, met by the horizontal pass (the line as a row) and by the vertical pass (the
    transposed image); the most negative accumulator must give byte 0 (arithmetic shift, lower clip), the largest byte 255"""
    bad = 0
    for n_in, n_out in case.RESIZE_AXES:
        t = case.tap_sign_lines(n_in, n_out, resample)
        assert -2 ** 31 <= t['acc_neg'] <= t['acc_pos'] < 2 ** 31
        image = case.tap_sign_image(n_in, n_out, resample)
        for label, im, size in (('rows', image, (5, n_out)), ('columns', np.ascontiguousarray(image.transpose(0, 2, 1)), (n_out, 5))):
            want = resize_ref.resize(im, size, resample)
            got = resize(im[None], size, resample)[0]
            n = int((got != want).sum())
            bad += n
            ends = (got[0, 0, t['xx_pos']], got[0, 1, t['xx_neg']]) if label == 'rows' else (got[0, t['xx_pos'], 0], got[0, t['xx_neg'], 1])
            print(f'{resample} {n_in}->{n_out} {label}: {n} of {want.size} bytes differ; accumulators {t["acc_neg"]} .. {t["acc_pos"]} give bytes '
                  f'{int(ends[1])} and {int(ends[0])}')
            assert ends == (255, 0), (n_in, n_out, label)
    assert bad == 0


@pytest.mark.parametrize('resample', case.FILTERS)
def test_resize_constants_stay_constant(resample):
    """B2: 256 constant images per call, each ratio on each axis; the twin holds the property (test_image_kernels_host.py)"""
    bad = {}
    for h, w, H, W in case.RESIZE_CONSTANT_SHAPES:
        images = case.constant_images(h, w)
        got = resize(images, (H, W), resample)
        off = [v for v in range(256) if (got[v] != v).any()]
        want = resize_ref.resize(images[:, 0], (H, W), resample)[:, None]        # the twin on the 256 images as 256 channels of one
        bad[h, w, H, W] = len(off) + int((got != want).sum())
        print(f'{resample} {h}x{w} -> {H}x{W}: {int((got != np.arange(256, dtype=np.uint8)[:, None, None, None]).sum())} of {got.size} bytes '
              f'leave their constant: {off[:16]}')
    assert not any(bad.values()), bad


@pytest.mark.parametrize('C', (1, 3))
@pytest.mark.parametrize('resample', case.FILTERS)
def test_resize_tile_edges_and_one_pixel_axes(resample, C):
    """B3: every output width around the 256-byte tile with every output height around the 4-row tile, one-pixel outputs, 8001 taps;
    `out` is a view at byte offsets 0..3 of a sentinel-filled buffer, and nothing may be written around it"""
    from cosypose_amd.resize import resize_images
    bad, spilled = {}, []
    for h, w, H, W, offset in case.resize_edge_shapes():
        images = case.resize_edge_images(h, w, C)
        want = resize_ref.resize_batch(images, (H, W), resample)
        buf, view = view_at(offset, want.shape)
        assert resize_images(dev(images), (H, W), resample, out=view) is view
        n = int((view.cpu().numpy() != want).sum())
        if n:
            bad[h, w, H, W, offset] = n
        if not untouched_around(buf, offset, want.size):
            spilled.append((h, w, H, W, offset))
    print(f'{resample} C={C}: shapes (h, w, H, W, offset) with bytes that differ: {bad}; written around `out`: {spilled}')
    assert not bad and not spilled


# ================================================================ C: frames
def frames_want(images, masks, H, W):
    n, _, h, w = images.shape
    return (frames_ref.image_bytes(images.reshape(-1, h, w), H, W).reshape(n, 3, H, W), np.stack([frames_ref.mask_nearest(m, H, W) for m in masks]))


def frames_check(label, images, masks, H, W, offset=None):
    from cosypose_amd.frames import resize_frames
    want, want_m = frames_want(images, masks, H, W)
    if offset is None:
        got = resize_frames(dev(images), (W, H), masks=dev(masks))
        spill = False
    else:
        buf, view = view_at(offset, want.shape)
        buf_m, view_m = view_at(offset, want_m.shape)
        got = resize_frames(dev(images), (W, H), masks=dev(masks), out=view, out_masks=view_m)
        assert got.images is view and got.masks is view_m
        spill = not (untouched_around(buf, offset, want.size) and untouched_around(buf_m, offset, want_m.size))
    bad, bad_m = int((got.images.cpu().numpy() != want).sum()), int((got.masks.cpu().numpy() != want_m).sum())
    print(f'{label}: {bad} of {want.size} image bytes and {bad_m} of {want_m.size} mask bytes differ from the definition'
          + ('' if offset is None else f'; out at byte offset {offset}, written around it: {spill}'))
    return bad + bad_m + int(spill)


def test_frames_every_byte_value_and_the_two_level_extremes():
    """C1: 256 constant frames per call at tiny sizes, a 0/255 checkerboard and a ramp at three ratios, masks that hold every id"""
    bad = 0
    for h, w, H, W in case.FRAME_CONSTANT_SHAPES:
        images, masks = case.frame_constants(h, w)
        bad += frames_check(f'constants {h}x{w} -> {H}x{W}', images, masks, H, W)
    for h, w, H, W in case.FRAME_STRUCTURED_SHAPES:
        images, masks = case.frame_structured(h, w)
        bad += frames_check(f'checkerboard and ramp {h}x{w} -> {H}x{W}', images, masks, H, W)
    assert bad == 0


@pytest.mark.parametrize('HW', tuple(case.FRAME_EDGE_SHAPES), ids=lambda s: f'{s[0]}x{s[1]}')
def test_frames_tile_edges_and_odd_addresses(HW):
    """C2: outputs around the 8-row x 128-byte tile from an up-scaling and a down-scaling source, noise and the seam frame; `out` and
    `out_masks` are views at byte offsets 1, 2 and 3 of sentinel-filled buffers"""
    bad = 0
    for h, w in case.FRAME_EDGE_SHAPES[HW]:
        images, masks = case.frame_edge_inputs(h, w)
        for offset in (1, 2, 3):
            bad += frames_check(f'{h}x{w} -> {HW[0]}x{HW[1]}', images, masks, *HW, offset=offset)
    assert bad == 0


def frames_by_hand(sources, H, W):
    """items and tables as cosypose_amd.frames.resize_frames lays them out, for a list of (image, mask) device tensors of one size
    -> items (numpy, ITEM_DTYPE), tables (numpy int32: the 256 byte values first)"""
    from cosypose_amd import frames
    from cosypose_amd._tables import TablePacker
    h, w = sources[0][0].shape[1:]
    packer = TablePacker(frames.byte_values())
    items = np.zeros(len(sources), frames.ITEM_DTYPE)
    items['image'], items['mask'] = [im.data_ptr() for im, _ in sources], [m.data_ptr() for _, m in sources]
    items['h'], items['w'] = h, w
    (items['xb'], items['xn']), (items['yb'], items['yn']) = frames.axis_offsets(packer, w, W), frames.axis_offsets(packer, h, H)
    return items, np.concatenate(packer.parts)


def upload(items, tables, shift_items=0, shift_tables=0):
    """one device buffer: the descriptors, then the tables at a multiple of 16 bytes (each moved by `shift_*` bytes) -> buffer, the two pointers"""
    items_bytes = -(-items.nbytes // 16) * 16 + 16
    blob = np.zeros(items_bytes + tables.nbytes + 32, np.uint8)
    blob[shift_items:shift_items + items.nbytes] = items.view(np.uint8)
    blob[items_bytes + shift_tables:items_bytes + shift_tables + tables.nbytes] = tables.view(np.uint8)
    blob_d = dev(blob)
    assert blob_d.data_ptr() % 16 == 0
    return blob_d, blob_d.data_ptr() + shift_items, blob_d.data_ptr() + items_bytes + shift_tables


def test_frames_descriptors_the_kernel_cannot_serve():
    """C3: one call with good frames at both ends and, between them, descriptors the kernel is written to skip: what it skips keeps the
    sentinel, every other plane equals the definition.  None of them asks the kernel to read outside a buffer."""
    from cosypose_amd import _lib
    lib = _lib.lib()
    h, w, H, W = 9, 12, 6, 8
    rs = np.random.RandomState(12)
    image, mask = rs.randint(0, 256, (3, h, w)).astype(np.uint8), rs.randint(0, 256, (h, w)).astype(np.uint8)
    want, want_m = frames_ref.image_bytes(image, H, W), frames_ref.mask_nearest(mask, H, W)
    image_d, mask_d = dev(image), dev(mask)
    # label -> (changed fields, image planes written, mask plane written)
    rows = (('good', {}, True, True), ('null image', dict(image=0), False, True), ('h = 0', dict(h=0), False, False),
            ('w = -1', dict(w=-1), False, False), ('xb = -4', dict(xb=-4), False, True), ('yb past the tables', dict(yb='end-4'), False, True),
            ('xb not a multiple of 4', dict(xb='+2'), False, True), ('yb not a multiple of 4', dict(yb='+1'), False, True),
            ('xn past the tables', dict(xn='end-W+1'), True, False), ('yn = -1', dict(yn=-1), True, False), ('null mask', dict(mask=0), True, False),
            ('good', {}, True, True))
    items, tables = frames_by_hand([(image_d, mask_d)] * len(rows), H, W)
    n_tables = int(tables.size)
    assert n_tables % 4 == 0
    for item, (_, changes, _, _) in zip(items, rows):
        for key, v in changes.items():
            item[key] = {'end-4': n_tables - 4, '+2': item[key] + 2, '+1': item[key] + 1, 'end-W+1': n_tables - W + 1}.get(v, v)
    blob_d, items_p, tables_p = upload(items, tables)
    out = torch.full((len(rows), 3, H, W), SENTINEL, dtype=torch.uint8, device='cuda')
    out_m = torch.full((len(rows), H, W), SENTINEL, dtype=torch.uint8, device='cuda')
    _lib.check(lib.cosy_resize_frames_u8(items_p, len(rows), H, W, tables_p, n_tables, 0, out.data_ptr(), out_m.data_ptr(), _lib.stream()))
    got, got_m = out.cpu().numpy(), out_m.cpu().numpy()
    wrong = []
    for i, (label, _, image_written, mask_written) in enumerate(rows):
        ok = np.array_equal(got[i], want) if image_written else bool((got[i] == SENTINEL).all())
        ok_m = np.array_equal(got_m[i], want_m) if mask_written else bool((got_m[i] == SENTINEL).all())
        if not (ok and ok_m):
            wrong.append((i, label, ok, ok_m))
    print(f'{len(rows)} descriptors, planes that are neither the definition where served nor untouched where skipped: {wrong}')
    assert not wrong
    # masks in the items and no out_masks: the images are written, no mask is
    out.fill_(SENTINEL)
    good, _ = frames_by_hand([(image_d, mask_d)] * 2, H, W)
    blob2_d, items2_p, tables2_p = upload(good, tables)
    _lib.check(lib.cosy_resize_frames_u8(items2_p, 2, H, W, tables2_p, n_tables, 0, out.data_ptr(), None, _lib.stream()))
    got = out.cpu().numpy()
    print(f'null out_masks: {int((got[:2] != want[None]).sum())} image bytes differ')
    assert np.array_equal(got[0], want) and np.array_equal(got[1], want) and (got[2:] == SENTINEL).all()


def test_frames_c_abi_refusals():
    """C3: cosy_resize_frames_u8 by hand: a refused call returns -1 and leaves both outputs untouched"""
    from cosypose_amd import _lib
    lib = _lib.lib()
    h, w, H, W, n = 9, 12, 6, 8, 2
    rs = np.random.RandomState(13)
    image_d, mask_d = dev(rs.randint(0, 256, (3, h, w)).astype(np.uint8)), dev(rs.randint(0, 256, (h, w)).astype(np.uint8))
    items, tables = frames_by_hand([(image_d, mask_d)] * n, H, W)
    n_tables = int(tables.size)
    blob_d, items_p, tables_p = upload(items, tables)
    shifted_t, _, tables_off = upload(items, tables, shift_tables=4)             # the same bytes, 4 bytes off a multiple of 16
    shifted_i, items_off, _ = upload(items, tables, shift_items=4)               # the same descriptors, 4 bytes off a multiple of 8
    assert tables_off % 16 == 4 and items_off % 8 == 4
    out = torch.full((n, 3, H, W), SENTINEL, dtype=torch.uint8, device='cuda')
    out_m = torch.full((n, H, W), SENTINEL, dtype=torch.uint8, device='cuda')
    call = Call(lib.cosy_resize_frames_u8, [out, out_m], items=items_p, n=n, H=H, W=W, tables=tables_p, n_tables=n_tables, lut=0,
                out_images=out.data_ptr(), out_masks=out_m.data_ptr(), stream=_lib.stream())
    bads = [dict(n=-1), dict(H=0), dict(W=0), dict(lut=-1), dict(lut=n_tables - 255), dict(n_tables=255), dict(n_tables=-1), dict(items=None),
            dict(tables=None), dict(out_images=None), dict(tables=tables_off), dict(items=items_off), dict(n=65535 // 4 + 1)]
    noops = [dict(n=0), dict(n=0, items=None, tables=None, out_images=None, out_masks=None)]
    call.check('cosy_resize_frames_u8', bads, noops)
    out.fill_(SENTINEL)
    out_m.fill_(SENTINEL)
    assert call() == 0
    want, want_m = frames_ref.image_bytes(image_d.cpu().numpy(), H, W), frames_ref.mask_nearest(mask_d.cpu().numpy(), H, W)
    bad = int((out.cpu().numpy() != want[None]).sum()) + int((out_m.cpu().numpy() != want_m[None]).sum())
    print(f'cosy_resize_frames_u8 by hand: {bad} bytes differ from the definition')
    assert bad == 0
