"""CPU tests of the image resize (cosypose_amd/resize.py, csrc/kernels_resize.hip): the numpy twin tests/resize_ref.py against the bytes
recorded from Pillow 12 (tests/golden/pillow_resize.npz) and, where PIL is installed, against live Pillow; the library's host routine
cosy_resize_coeffs against the twin's tables, integer for integer; the C ABI; the build flags; the refusals that need no device.  Every
comparison is np.array_equal: there is no tolerance in this file."""
import ctypes
import re

import numpy as np
import pytest

import resize_ref
from conftest import REPO

FILTERS = ('bilinear', 'bicubic')
SHAPES = {(1, 1, 4, 5), (2, 3, 5, 7), (3, 2, 1, 1), (5, 7, 5, 9), (5, 7, 8, 7), (24, 32, 24, 32), (37, 53, 48, 64), (97, 211, 24, 32),
          (131, 67, 70, 150), (300, 8, 6, 8)}


@pytest.fixture(scope='module')
def golden_resize():
    return resize_ref.golden_cases(REPO / 'tests' / 'golden' / 'pillow_resize.npz')


@pytest.fixture(scope='module')
def hostlib():
    from cosypose_amd.build import build, LIB
    build()
    lib = ctypes.CDLL(LIB)
    lib.cosy_resize_ksize.restype, lib.cosy_resize_ksize.argtypes = ctypes.c_int, [ctypes.c_int] * 3
    lib.cosy_resize_coeffs.restype = ctypes.c_int
    lib.cosy_resize_coeffs.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    return lib


def host_coeffs(lib, n_in, n_out, resample):
    filt = resize_ref.FILTERS[resample]
    ksize = lib.cosy_resize_ksize(n_in, n_out, filt)
    assert ksize > 0
    bounds, k = np.full((n_out, 2), -7, np.int32), np.full((n_out, ksize), -7, np.int32)
    assert lib.cosy_resize_coeffs(n_in, n_out, filt, bounds.ctypes.data, k.ctypes.data, k.size) == ksize
    return bounds, k


def test_fixture_covers_what_it_is_for(golden_resize):
    cases, g = golden_resize
    assert str(g['pil_version'].reshape(-1)[0]) == '12.2.0'
    assert [str(c) for c in g['contents']] == ['random', 'zeros', 'ones', 'checkerboard']
    got = {c['images'].shape[2:] + c['size'] for c in cases.values() if c['images'].shape[1] == 3}
    assert got == SHAPES
    assert sum(c['images'].shape[1] == 1 for c in cases.values()) == 2
    for name, c in cases.items():
        im = c['images']
        assert im.dtype == np.uint8 and len(im) == 4 and not im[1].any() and (im[2] == 255).all() and set(np.unique(im[3])) <= {0, 255}, name
        assert c['bicubic'].shape == c['bilinear'].shape == im.shape[:2] + c['size'], name
    # the checkerboard under bicubic reaches both clips (before the clip the twin sees values below 0 and above 255), a constant image
    # stays constant, an image at size is a copy
    big = cases['131x67_to_70x150']
    raw = []
    assert np.array_equal(resize_ref.resize(big['images'][3], big['size'], 'bicubic', raw), big['bicubic'][3])
    assert min(raw) < 0 and max(raw) > 255 and len(np.unique(big['bicubic'][3])) > 2
    assert not big['bicubic'][1].any() and (big['bicubic'][2] == 255).all()
    same = cases['24x32_to_24x32']
    assert np.array_equal(same['bicubic'], same['images']) and np.array_equal(same['bilinear'], same['images'])
    # up to 29 taps on the 211 -> 32 axis, 201 on the 300 -> 6 one
    assert resize_ref.coeffs(211, 32, 'bicubic')[1].shape[1] == 29 and resize_ref.coeffs(300, 6, 'bicubic')[1].shape[1] == 201


def test_twin_equals_pillow_on_every_case(golden_resize):
    cases, _ = golden_resize
    bad = {}
    for name, c in cases.items():
        for f in FILTERS:
            got = resize_ref.resize_batch(c['images'], c['size'], f)
            bad[name, f] = int((got != c[f]).sum())
    print(bad)
    assert len(bad) == 24 and not any(bad.values()), bad


def test_twin_equals_live_pillow_on_seeded_shapes():
    PIL = pytest.importorskip('PIL')
    from PIL import Image
    rs = np.random.RandomState(5)
    shapes = [(375, 500, 480, 640), (9, 1, 3, 17), (1, 40, 6, 6), (64, 64, 63, 65)] + [tuple(rs.randint(1, 90, 4)) for _ in range(12)]
    for h, w, H, W in shapes:
        for binary in (False, True):
            im = (rs.randint(0, 2, (3, h, w)) * 255 if binary else rs.randint(0, 256, (3, h, w))).astype(np.uint8)
            pil = Image.fromarray(np.ascontiguousarray(im.transpose(1, 2, 0)))
            for f, filt in (('bilinear', Image.BILINEAR), ('bicubic', Image.BICUBIC)):
                want = np.asarray(pil.resize((int(W), int(H)), filt)).transpose(2, 0, 1)
                assert np.array_equal(resize_ref.resize(im, (int(H), int(W)), f), want), (h, w, H, W, f, binary, PIL.__version__)
            assert np.array_equal(np.asarray(pil.resize((int(W), int(H)))), np.asarray(pil.resize((int(W), int(H)), Image.BICUBIC)))


def test_host_coefficients_equal_the_twin_on_every_axis(golden_resize, hostlib):
    cases, _ = golden_resize
    axes = {(c['images'].shape[3], c['size'][1]) for c in cases.values()} | {(c['images'].shape[2], c['size'][0]) for c in cases.values()}
    axes |= {(500, 640), (375, 480), (333, 480), (500, 480), (334, 640), (7, 7)}
    assert len(axes) >= 20
    for n_in, n_out in sorted(axes):
        for f in FILTERS:
            bounds, k = host_coeffs(hostlib, n_in, n_out, f)
            want_b, want_k = resize_ref.coeffs(n_in, n_out, f)
            assert np.array_equal(bounds, want_b), (n_in, n_out, f)
            assert k.shape == want_k.shape and np.array_equal(k, want_k), (n_in, n_out, f)
            assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] <= k.shape[1]).all() and (bounds.sum(axis=1) <= n_in).all()


def test_host_routine_refuses_what_it_cannot_serve(hostlib):
    lib = hostlib
    buf = np.zeros(64, np.int32)
    assert lib.cosy_resize_ksize(0, 4, 3) < 0 and lib.cosy_resize_ksize(4, 0, 3) < 0 and lib.cosy_resize_ksize(4, 4, 0) < 0
    assert lib.cosy_resize_ksize(4, 4, 1) < 0                                   # Image.LANCZOS: not served
    assert lib.cosy_resize_ksize(300, 6, 3) == 201 and lib.cosy_resize_ksize(5, 9, 2) == 3 and lib.cosy_resize_ksize(5, 9, 3) == 5
    before = buf.copy()
    assert lib.cosy_resize_coeffs(5, 9, 3, buf.ctypes.data, buf.ctypes.data + 128, 9 * 5 - 1) < 0      # capacity one short
    assert np.array_equal(buf, before)
    assert lib.cosy_resize_coeffs(5, 9, 3, None, buf.ctypes.data, 64) < 0


def test_c_abi_exports_the_resize_entry_points(hostlib):
    from cosypose_amd import _lib, resize
    for name in ('cosy_resize_ksize', 'cosy_resize_coeffs', 'cosy_resize_workspace_bytes', 'cosy_resize_u8'):
        assert name in _lib.EXPORTS, name           # test_c_abi.py: EXPORTS, the header and the built library name the same entry points,
                                                    # the COSY_RESIZE_* values and cosy_resize_item_t field by field
    assert resize.FILTERS == resize_ref.FILTERS
    f = hostlib.cosy_resize_workspace_bytes
    f.restype, f.argtypes = ctypes.c_size_t, [ctypes.c_int] * 4
    assert f(64, 3, 500, 640) >= 64 * 3 * 500 * 640 and f(0, 3, 500, 640) == 0
    import cosypose_amd
    assert cosypose_amd.resize_images is resize.resize_images
    # the Python side reads its tables from the library, and keeps them
    bounds, k = resize.axis_tables(211, 32, 'bicubic')
    want_b, want_k = resize_ref.coeffs(211, 32, 'bicubic')
    assert np.array_equal(bounds, want_b) and np.array_equal(k, want_k) and resize.axis_tables(211, 32, 'bicubic')[1] is k
    assert not k.flags.writeable


def test_resize_source_is_built_with_contraction_off():
    from cosypose_amd import build
    assert 'kernels_resize.hip' in build.SOURCES
    assert '-ffp-contract=off' in build.FILE_FLAGS['kernels_resize.hip']
    text = (REPO / 'cosypose_amd' / 'csrc' / 'kernels_resize.hip').read_text()
    assert '#pragma clang fp contract(off)' in text


def test_resize_kernels_hold_no_floating_point(hostlib):
    """the device side is integer arithmetic only: no half, float or double instruction in the disassembly of the shipped object"""
    import os
    import subprocess
    import tempfile
    from cosypose_amd import build as hipbuild
    llvm = '/opt/rocm/lib/llvm/bin/'
    if not os.path.exists(llvm + 'llvm-objdump'):
        pytest.skip('needs the ROCm llvm tools')
    with tempfile.TemporaryDirectory() as tmp:
        co, fat = os.path.join(tmp, 'dev.co'), os.path.join(tmp, 'fat.bin')
        subprocess.run([llvm + 'llvm-objcopy', f'--dump-section=.hip_fatbin={fat}', hipbuild._obj('kernels_resize.hip')], check=True)
        subprocess.run([llvm + 'clang-offload-bundler', '--unbundle', '--type=o', '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', f'--input={fat}',
                        f'--output={co}'], check=True)
        asm = subprocess.run([llvm + 'llvm-objdump', '-d', co], capture_output=True, text=True).stdout
    assert 'resize_rows_kernel' in asm and 'resize_cols_kernel' in asm
    assert 'v_mad_' in asm or 'v_mul_' in asm
    assert not re.findall(r'\bv_\w*_f(?:16|32|64)\w*', asm)


def test_resize_images_refuses_cpu_tensors_and_malformed_arguments():
    torch = pytest.importorskip('torch')
    from cosypose_amd import _lib
    from cosypose_amd.resize import resize_images
    im = torch.zeros(2, 3, 5, 7, dtype=torch.uint8)
    with pytest.raises(_lib.CosyHipError, match='no CPU fallback'):
        resize_images(im, (4, 4))
    with pytest.raises(_lib.CosyHipError, match='no CPU fallback'):
        resize_images([im[0], im[1]], (4, 4))
    for size in ((0, 4), (4, -1), (4,), 4, (4.5, 4)):
        with pytest.raises(ValueError, match='size'):
            resize_images(im, size)
    for name in ('nearest', 'lanczos', 3):
        with pytest.raises(ValueError, match='resample'):
            resize_images(im, (4, 4), resample=name)
    # what follows is checked before the library is touched; a meta tensor stands in for a device one
    meta = lambda *shape, dtype=torch.uint8: torch.empty(*shape, dtype=dtype, device='meta')
    fake = lambda *tensors: None
    import unittest.mock
    with unittest.mock.patch.object(_lib, 'require_device', fake):
        with pytest.raises(ValueError, match='uint8'):
            resize_images(meta(2, 3, 5, 7, dtype=torch.float32), (4, 4))
        with pytest.raises(ValueError, match='uint8'):
            resize_images(meta(3, 5, 7), (4, 4))                        # rank 3 is one image of a list, not a batch
        with pytest.raises(ValueError, match='uint8'):
            resize_images([meta(2, 3, 5, 7)], (4, 4))
        with pytest.raises(ValueError, match='uint8'):
            resize_images([meta(3, 5, 7, dtype=torch.int32)], (4, 4))
        with pytest.raises(ValueError, match='1 or 3 channels'):
            resize_images(meta(2, 2, 5, 7), (4, 4))
        with pytest.raises(ValueError, match='1 or 3 channels'):
            resize_images([meta(4, 5, 7)], (4, 4))
        with pytest.raises(ValueError, match='same number of channels'):
            resize_images([meta(3, 5, 7), meta(1, 5, 7)], (4, 4))
        with pytest.raises(ValueError, match='out must be'):
            resize_images(meta(2, 3, 5, 7), (4, 4), out=meta(2, 3, 4, 5))
        with pytest.raises(ValueError, match='without pixels'):
            resize_images(meta(2, 3, 0, 7), (4, 4))
