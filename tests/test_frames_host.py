"""CPU tests of the frames' own resize (cosypose_amd/frames.py, csrc/kernels_frames.hip): the numpy restatement
tests/frames_ref.py against what the reference's CropResizeToAspectAugmentation gave (tests/golden/reference_golden_frames.npz) under
section 18's parity rule, and against torch's generic bilinear kernel float for float; the tables the package computes on the host
against the restatement's, bit for bit; the C ABI; the refusals that need no device.

The parity rule: the reference's bytes depend on which of torch's kernels ran wherever the exact value of a byte is an integer, so
  * no byte differs outside the set of bytes whose float64-exact value lies within 1e-4 of an integer, and that set holds at most 1 % of a case;
  * inside it the difference is at most one level;
  * masks, boxes and crop_resize_bbox are equal, K is within 2e-6 relative."""
import re

import numpy as np
import pytest

import frames_ref
from conftest import REPO, rel_err

CASES = ('99x132_to_48x64', '45x60_to_48x64', '54x72_to_48x64', '150x200_to_96x128', '50x50_to_32x32', '48x64_to_48x64')
MAX_NEAR_SHARE = 0.01
K_TOL = 2e-6


@pytest.fixture(scope='module')
def golden_frames():
    g = np.load(REPO / 'tests' / 'golden' / 'reference_golden_frames.npz')
    return {str(name): {key: g[f'{name}_{key}'] for key in ('image', 'mask', 'K', 'resize', 'out_image', 'out_mask', 'out_K', 'bbox', 'boxes', 'resized')}
            for name in g['cases']}, g


def test_fixture_covers_what_it_is_for(golden_frames):
    cases, g = golden_frames
    assert tuple(cases) == CASES and int(g['n_ids'].reshape(-1)[0]) == 6 and int(g['absent_id'].reshape(-1)[0]) == 4
    for name, c in cases.items():
        h, w, H, W = (int(v) for v in re.fullmatch(r'(\d+)x(\d+)_to_(\d+)x(\d+)', name).groups())
        assert c['image'].shape == (3, h, w) and c['mask'].shape == (h, w) and c['out_image'].shape == (3, H, W) and c['out_mask'].shape == (H, W), name
        assert frames_ref.out_size(c['resize']) == (H, W) and bool(c['resized']) == ((h, w) != (H, W)), name
        assert sorted(np.unique(c['mask'])) == [0, 1, 2, 3, 5], name                    # five ids, id 4 absent
        assert c['mask'][0, 0] == 1, name                                               # id 1 touches the border
        if c['resized']:
            assert tuple(c['boxes'][1][:2]) == (0, 0) and (c['boxes'][4] == -1).all() and (c['boxes'][[0, 1, 2, 3, 5]] >= 0).all(), name
    assert [n for n, c in cases.items() if not c['resized']] == ['48x64_to_48x64']
    assert cases['45x60_to_48x64']['image'].shape[1] < 48                               # an upscale is among them


@pytest.mark.parametrize('name', CASES)
def test_restatement_against_the_reference(golden_frames, name):
    c = golden_frames[0][name]
    H, W = frames_ref.out_size(c['resize'])
    got = frames_ref.resize_frame(c['image'], c['resize'], c['mask'], c['K'])
    assert got['resized'] == bool(c['resized'])
    if got['resized']:
        outside, inside, share = frames_ref.parity_report(got['image'], c['out_image'], frames_ref.image_exact(c['image'], H, W))
        print(f'{name}: {outside} bytes differ outside the near-integer set, largest difference inside {inside}, share {100 * share:.3f} %')
        assert outside == 0 and inside <= 1 and share <= MAX_NEAR_SHARE
        assert np.array_equal(frames_ref.instance_stats(got['mask'], 6)[:, 1:], c['boxes'])
    else:
        assert np.array_equal(got['image'], c['out_image']) and np.array_equal(got['image'], c['image'])
        assert (c['boxes'][[0, 1, 2, 3, 5]] == -7).all()                                 # the reference left the boxes it was given
    assert np.array_equal(got['mask'], c['out_mask'])
    assert got['crop_resize_bbox'] == tuple(c['bbox'])
    assert got['K'].dtype == np.float32 and rel_err(got['K'], c['out_K']) < K_TOL


def test_restatement_floats_are_torchs_generic_kernel():
    """torch takes its generic (not channels-last, not vectorised) bilinear kernel for a contiguous NCHW input, more than one thread and
    an output with H + W > 128: there the restatement gives the same float32 everywhere"""
    import os
    torch = pytest.importorskip('torch')
    import torch.nn.functional as F
    if (os.cpu_count() or 1) < 2:
        pytest.skip('the host has one core: torch would run its single-thread vectorised kernel, which section 18 does not restate')
    before = torch.get_num_threads()
    torch.set_num_threads(2)
    try:
        if torch.get_num_threads() < 2:
            pytest.skip('torch runs on one thread here: it would take its vectorised kernel, which section 18 does not restate')
        rs = np.random.RandomState(18)
        image = rs.randint(0, 256, (3, 150, 200)).astype(np.uint8)
        image[:, :40, :50], image[:, 100:, 150:] = 255, 77                              # flat regions: every byte there is near-integer
        x = (torch.from_numpy(image).float() / 255).unsqueeze(0).contiguous()
        want = F.interpolate(x, size=(96, 128), mode='bilinear', align_corners=False)[0]
        want_mask = F.interpolate(torch.from_numpy(image[:1, None].astype(np.float32)), size=(96, 128), mode='nearest')[0, 0]
    finally:
        torch.set_num_threads(before)
    got = torch.from_numpy(frames_ref.image_float(image, 96, 128))
    print('floats that differ:', int((got != want).sum()), 'of', got.numel())
    assert torch.equal(got, want)
    assert np.array_equal(frames_ref.to_bytes(got.numpy()), (want * 255).to(torch.uint8).numpy())
    assert np.array_equal(frames_ref.mask_nearest(image[0], 96, 128), want_mask.numpy().astype(np.uint8))


def test_fma_emulation_names_the_sums_it_cannot_round():
    F32 = np.float32
    # exact float64 sums are rounded once, a float32 midpoint among them: 1 + 2^-24 ties to even
    assert frames_ref.fma32(F32(1), F32(1), F32(2.0 ** -24)) == F32(1)
    assert frames_ref.fma32(F32(0.75), F32(0.2), F32(0.25) * F32(0.2)) == F32(0.2)
    # (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 is a float32 midpoint and exact in float64: alone it ties to even ...
    a = F32(1 + 2.0 ** -12)
    assert frames_ref.fma32(a, a, F32(0)) == F32(1 + 2.0 ** -11)
    # ... but with 2^-70 added the true sum lies above the midpoint while the float64 sum does not: the emulation would round down
    with pytest.raises(frames_ref.DoubleRounding):
        frames_ref.fma32(a, a, F32(2.0 ** -70))
    with pytest.raises(frames_ref.DoubleRounding, match='1 sums'):
        frames_ref.fma32(np.array([0.5, a], F32), np.array([0.5, a], F32), np.array([0.25, -2.0 ** -70], F32))


def test_host_tables_equal_the_restatement():
    from cosypose_amd import frames
    for n_in, n_out in ((1, 3), (1, 4), (3, 12), (4, 16), (96, 48), (99, 48), (132, 64), (150, 96), (200, 128), (50, 32), (240, 48), (320, 64),
                        (33, 22), (45, 30), (540, 480), (720, 640), (960, 480), (1280, 640)):
        taps, nearest = frames.axis_tables(n_in, n_out)
        i0, i1, l0, l1 = frames_ref.axis(n_in, n_out)
        assert taps.dtype == np.int32 and taps.shape == (n_out, 4) and nearest.dtype == np.int32 and not taps.flags.writeable
        assert np.array_equal(taps[:, 0], i0) and np.array_equal(taps[:, 1], i1)
        assert np.array_equal(taps[:, 2], l0.view(np.int32)) and np.array_equal(taps[:, 3], l1.view(np.int32))
        assert np.array_equal(nearest, frames_ref.nearest_index(n_in, n_out))
        assert 0 <= i0.min() and i1.max() <= n_in - 1 and 0 <= nearest.min() and nearest.max() <= n_in - 1
        assert frames.axis_tables(n_in, n_out)[0] is taps
    assert np.array_equal(frames.byte_values().view(np.float32), (np.arange(256, dtype=np.float32) / np.float32(255)))
    rs = np.random.RandomState(3)
    for h, w, H, W in ((540, 720, 480, 640), (960, 1280, 480, 640), (45, 60, 48, 64), (50, 50, 32, 32)):
        K = np.array([[rs.uniform(500, 1500), 0, w / 2 + rs.uniform(-9, 9)], [0, rs.uniform(500, 1500), h / 2 + rs.uniform(-9, 9)], [0, 0, 1]])
        got = frames.resized_K(K, h, w, H, W)
        assert got.dtype == np.float32 and np.array_equal(got, frames_ref.K_resize(K, h, w, H, W))


def test_table_packer_layout_is_pinned():
    """the one buffer of a host-packed call (cosypose_amd/_tables.py), on 3 -> 2 and 5 -> 4 behind the 256 byte values: every offset as a
    literal, the bytes of the buffer against the parts, the descriptor block rounded to 16 bytes"""
    from cosypose_amd import frames
    from cosypose_amd._tables import TablePacker
    packer = TablePacker(frames.byte_values())
    assert frames.axis_offsets(packer, 3, 2) == (256, 264) and packer.size == 268          # 8 tap ints, 2 nearest, 2 of padding
    assert frames.axis_offsets(packer, 5, 4) == (268, 284) and packer.size == 288          # 16 tap ints, 4 nearest, none
    assert frames.axis_offsets(packer, 3, 2) == (256, 264) and packer.size == 288          # a repeated key is placed once
    assert packer.place('a', np.arange(3, dtype=np.int32), align_ints=4) == (288,) and packer.size == 292
    assert packer.append(np.array([(0, 0), (0, 1), (2, 0)], np.int32)) == 292 and packer.size == 298      # the detector's units: no padding
    assert packer.place('b', np.zeros((2, 4), np.int32), np.zeros(2, np.int32), align_ints=4) == (300, 308) and packer.size == 312
    assert all(at % 4 == 0 for at in (256, 268, 300))                                      # every tap table at a multiple of 4 ints
    (t32, n32), (t54, n54) = frames.axis_tables(3, 2), frames.axis_tables(5, 4)
    want = np.concatenate([frames.byte_values(), t32.reshape(-1), n32, [0, 0], t54.reshape(-1), n54, [0, 1, 2, 0], [0, 0, 0, 1, 2, 0], np.zeros(14)])
    assert want.size == 312
    for n, at in ((1, 48), (2, 80), (3, 128), (4, 160)):                                   # descriptors of 40 bytes
        items = np.zeros(n, frames.ITEM_DTYPE)
        items['h'], items['w'], items['image'] = 3 + np.arange(n), 5, 0x0102030405060708
        blob, tables_at, n_tables = packer.blob(items)
        assert (tables_at, n_tables) == (at, 312) and tables_at % 16 == 0
        assert blob.dtype == np.uint8 and blob.size == at + 4 * 312
        assert blob[:40 * n].tobytes() == items.tobytes() and not blob[40 * n:at].any()
        assert blob[at:].tobytes() == want.astype(np.int32).tobytes()
    # no head, no padding asked for, as resize_images packs; and never an empty table: one zero stands for none
    bare = TablePacker(what='coefficient tables')
    assert bare.blob(np.zeros(1, frames.ITEM_DTYPE))[1:] == (48, 1) and bare.blob(np.zeros(1, frames.ITEM_DTYPE))[0].size == 52
    assert bare.place((7, 5), np.ones((5, 2), np.int32), np.ones((5, 3), np.int32)) == (0, 10) and bare.size == 25
    assert bare.place((9, 5), np.ones((5, 2), np.int32), np.ones((5, 4), np.int32)) == (25, 35) and bare.size == 55
    assert bare.blob(np.zeros(2, frames.ITEM_DTYPE))[1:] == (80, 55)
    for p, text in ((packer, r'the tables of this call exceed 2\^31 entries'), (bare, r'the coefficient tables of this call exceed 2\^31 entries')):
        p.size = 2 ** 31
        with pytest.raises(ValueError, match=text):
            p.blob(np.zeros(1, frames.ITEM_DTYPE))


def test_c_abi_exports_the_frames_entry_point():
    import cosypose_amd
    from cosypose_amd import _lib, build, frames
    assert 'cosy_resize_frames_u8' in _lib.EXPORTS           # test_c_abi.py: EXPORTS, the header and the built library name the same entry points, cosy_frame_item_t field by field
    assert 'kernels_frames.hip' in build.SOURCES and '-ffp-contract=off' in build.FILE_FLAGS['kernels_frames.hip']
    assert cosypose_amd.resize_frames is frames.resize_frames


def test_frames_kernel_fuses_what_section_18_fuses_and_divides_nothing():
    """in the shipped object the kernel holds fused multiply-adds and lone products, no unfused multiply-add and no division"""
    import os
    import subprocess
    import tempfile
    from cosypose_amd import build as hipbuild
    hipbuild.build()
    llvm = '/opt/rocm/lib/llvm/bin/'
    if not os.path.exists(llvm + 'llvm-objdump'):
        pytest.skip('needs the ROCm llvm tools')
    with tempfile.TemporaryDirectory() as tmp:
        co, fat = os.path.join(tmp, 'dev.co'), os.path.join(tmp, 'fat.bin')
        subprocess.run([llvm + 'llvm-objcopy', f'--dump-section=.hip_fatbin={fat}', hipbuild._obj('kernels_frames.hip')], check=True)
        subprocess.run([llvm + 'clang-offload-bundler', '--unbundle', '--type=o', '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', f'--input={fat}',
                        f'--output={co}'], check=True)
        asm = subprocess.run([llvm + 'llvm-objdump', '-d', co], capture_output=True, text=True).stdout
    assert 'resize_frames_kernel' in asm
    fused = re.findall(r'\bv_fma(?:c)?_f32\w*', asm)
    products = re.findall(r'\bv_mul_f32\w*', asm)
    print(len(fused), 'fused multiply-adds,', len(products), 'products')
    assert len(fused) == 12 and len(products) == 16                                     # per thread: 4 bytes x (3 fma, 3 + 1 products)
    assert not re.findall(r'\bv_(?:mad|mac|rcp|div|add|sub)\w*_f(?:16|32|64)\w*', asm)


def test_resize_frames_refuses_cpu_tensors_and_malformed_arguments():
    torch = pytest.importorskip('torch')
    import unittest.mock
    from cosypose_amd import _lib, frames
    from cosypose_amd.frames import resize_frames
    im = torch.zeros(2, 3, 6, 8, dtype=torch.uint8)
    with pytest.raises(_lib.CosyHipError, match='no CPU fallback'):
        resize_frames(im, (4, 3))
    with pytest.raises(_lib.CosyHipError, match='no CPU fallback'):
        resize_frames([im[0], im[1]], (4, 3))
    for resize in ((0, 4), (4, -1), (4,), 4, (4.5, 4)):
        with pytest.raises(ValueError, match='resize'):
            resize_frames(im, resize)
    with pytest.raises(ValueError, match=r'frame 3 is 13x16.*1\.23077.*1\.33333'):
        frames.check_aspect(3, 13, 16, 48, 64)
    frames.check_aspect(0, 33, 45, 22, 30)
    frames.check_aspect(0, 50, 50, 32, 32)
    # what follows is checked before the library is touched; a meta tensor stands in for a device one
    meta = lambda *shape, dtype=torch.uint8: torch.empty(*shape, dtype=dtype, device='meta')
    with unittest.mock.patch.object(_lib, 'require_device', lambda *tensors: None):
        with pytest.raises(ValueError, match='uint8'):
            resize_frames(meta(2, 3, 6, 8, dtype=torch.float32), (4, 3))
        with pytest.raises(ValueError, match='uint8'):
            resize_frames(meta(3, 6, 8), (4, 3))                          # rank 3 is one frame of a list, not a batch
        with pytest.raises(ValueError, match='uint8'):
            resize_frames([meta(2, 3, 6, 8)], (4, 3))
        with pytest.raises(ValueError, match='uint8'):
            resize_frames([np.zeros((3, 6, 8), np.uint8)], (4, 3))
        with pytest.raises(ValueError, match='3 channels'):
            resize_frames(meta(2, 1, 6, 8), (4, 3))
        with pytest.raises(ValueError, match='at least one frame'):
            resize_frames([], (4, 3))
        with pytest.raises(ValueError, match='without pixels'):
            resize_frames(meta(2, 3, 0, 8), (4, 3))
        with pytest.raises(ValueError, match=r'frame 1 is 6x9'):
            resize_frames([meta(3, 6, 8), meta(3, 6, 9)], (4, 3))
        with pytest.raises(ValueError, match='one .* mask per frame'):
            resize_frames(meta(2, 3, 6, 8), (4, 3), masks=meta(1, 6, 8))
        with pytest.raises(ValueError, match='one .* mask per frame'):
            resize_frames(meta(2, 3, 6, 8), (4, 3), masks=[meta(6, 8), meta(3, 4)])
        with pytest.raises(ValueError, match='uint8'):
            resize_frames(meta(2, 3, 6, 8), (4, 3), masks=meta(2, 6, 8, dtype=torch.int32))
        with pytest.raises(ValueError, match='need masks'):
            resize_frames(meta(2, 3, 6, 8), (4, 3), boxes=True)
        with pytest.raises(ValueError, match='need masks'):
            resize_frames(meta(2, 3, 6, 8), (4, 3), out_masks=meta(2, 3, 4))
        with pytest.raises(ValueError, match=r'K must be \(2,3,3\)'):
            resize_frames(meta(2, 3, 6, 8), (4, 3), K=np.zeros((3, 3)))
        with pytest.raises(ValueError, match='out must be'):
            resize_frames(meta(2, 3, 6, 8), (4, 3), out=meta(2, 3, 4, 3))
        with pytest.raises(ValueError, match='out_masks must be'):
            resize_frames(meta(2, 3, 6, 8), (4, 3), masks=meta(2, 6, 8), out_masks=meta(2, 3, 5))
