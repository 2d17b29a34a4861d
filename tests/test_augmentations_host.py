"""CPU tests of the training augmentations (cosypose_amd/augmentations.py, csrc/kernels_aug.hip): the numpy twin tests/aug_ref.py against
every stage output recorded from the reference's classes under Pillow (tests/golden/reference_golden_aug.npz), the host-side draws
against the recorded draw sequences, the parameter table, the C ABI, and the absence of fused multiply-adds in the compiled kernels."""
import ctypes
import os
import random
import re
import subprocess
import tempfile

import numpy as np
import pytest

import aug_ref
from conftest import REPO

KIND = {'random': 0, 'randint': 1, 'uniform': 2}


@pytest.fixture(scope='module')
def golden_aug():
    return aug_ref.golden_cases(REPO / 'tests' / 'golden' / 'reference_golden_aug.npz')


def test_fixture_covers_what_it_is_for(golden_aug):
    cases, g = golden_aug
    sizes = {c['images'].shape[2:] for c in cases.values()}
    assert {(1, 1), (2, 3), (3, 3), (5, 7), (37, 53), (48, 64), (67, 131)} <= sizes
    recs = [r for c in cases.values() for r in c['recs']]
    assert {r['k'] for r in recs if r['gate']} == {1, 2, 3} and any(not r['gate'] for r in recs)
    for name, ends in (('sharpness', (0., 50.)), ('contrast', (0.2, 50.)), ('brightness', (0.1, 6.)), ('color', (0., 20.))):
        factors = {r[name] for r in recs if r[name] is not None}
        assert set(ends) | {1.0} <= factors and any(r['gate'] and r[name] is None for r in recs), name
    assert {0.0} <= {r['contrast'] for r in recs if r['contrast'] is not None} and {0.0} <= {r['brightness'] for r in recs if r['brightness'] is not None}
    half = cases['halfmean_5x6']                 # the image Contrast sees has a mean L of exactly x.5
    l = aug_ref.luma(half['stages']['blur'][1][0].transpose(1, 2, 0)).astype(np.int64)
    assert 2 * int(l.sum()) % (2 * l.size) == l.size


def test_twin_equals_every_recorded_stage(golden_aug):
    cases, g = golden_aug
    assert str(g['pil_version'].reshape(-1)[0]).split('.')[0] == '12'
    n_stage = 0
    for name, c in cases.items():
        for b, rec in enumerate(c['recs']):
            stages = []
            out = aug_ref.augment_one(np.ascontiguousarray(c['images'][b].transpose(1, 2, 0)), rec, c['masks'][b], c['backgrounds'], stages)
            ran = {st for st, (idx, _) in c['stages'].items() if b in idx}
            assert {st for st, _ in stages} == ran, (name, b)
            for st, im in stages:
                idx, want = c['stages'][st]
                assert np.array_equal(im.transpose(2, 0, 1), want[list(idx).index(b)]), (name, b, st)
                n_stage += 1
            assert np.array_equal(out.transpose(2, 0, 1), c['out'][b]), (name, b)
        assert np.array_equal(aug_ref.augment(c['images'], c['recs'], c['masks'], c['backgrounds']), c['out']), name
    assert n_stage > 150


class _Recording:
    def __init__(self):
        self.log = []

    def random(self):
        self.log.append((0, random.random()))
        return self.log[-1][1]

    def randint(self, a, b):
        self.log.append((1, random.randint(a, b)))
        return self.log[-1][1]

    def uniform(self, a, b):
        self.log.append((2, random.uniform(a, b)))
        return self.log[-1][1]


def test_draw_sample_params_makes_the_recorded_draws(golden_aug):
    from cosypose_amd.augmentations import draw_sample_params
    cases, g = golden_aug
    state = random.getstate()
    try:
        for s in g['seeds']:
            c, draws = cases[f'seed{s}'], g[f'seed{s}_draws']
            random.seed(int(s))
            for b, want in enumerate(c['recs']):
                rng = _Recording()
                rec = draw_sample_params(rng, rgb_augmentation=True, gray_augmentation=True, background_p=0.3, n_backgrounds=len(c['backgrounds']))
                n = int((~np.isnan(draws[b, :, 0])).sum())
                assert len(rng.log) == n and all(k == draws[b, j, 0] and v == draws[b, j, 1] for j, (k, v) in enumerate(rng.log)), (s, b)
                assert rec == want, (s, b, rec, want)
            assert random.random() == float(g[f'seed{s}_next'].reshape(-1)[0]), s            # the generator is left where the reference leaves it
        # the module itself is the default source, and the switches remove exactly their draws
        random.seed(5)
        a = draw_sample_params(n_backgrounds=2, gray_augmentation=True)
        random.seed(5)
        assert a == draw_sample_params(random.Random(5), n_backgrounds=2, gray_augmentation=True) and random.random() == random.Random(5).random()
        r = random.Random(9)
        assert draw_sample_params(r, rgb_augmentation=False) == dict(bg=-1, gate=False, k=0, sharpness=None, contrast=None, brightness=None,
                                                                      color=None, gray=False)
        assert r.random() == random.Random(9).random()
    finally:
        random.setstate(state)


def test_pack_params_round_trip(golden_aug):
    from cosypose_amd import augmentations as aug
    cases, _ = golden_aug
    recs = [r for c in cases.values() for r in c['recs']]
    table = aug.pack_params(recs)
    assert table.dtype.itemsize == 32 and table.shape == (len(recs),)
    back = aug.unpack_params(table)
    for r, b in zip(recs, back):
        want = dict(r, **{n: None if r[n] is None else float(np.float32(r[n])) for n in aug_ref.STAGES})
        assert b == want
    assert np.array_equal(aug.pack_params(back), table)
    raw = table.view(np.int32).reshape(-1, 8)                      # the layout of cosy_aug_params_t
    first = next(i for i, r in enumerate(recs) if r['gate'] and r['contrast'] is not None)
    assert raw[first, 1] & aug.GATE and raw[first, 1] & aug.CONTRAST and raw[first, 2] == recs[first]['k']
    assert raw[first, 4:5].view(np.float32)[0] == np.float32(recs[first]['contrast'])
    with pytest.raises(ValueError):
        aug.pack_params([dict(recs[first], k=4)])
    with pytest.raises(ValueError):
        aug.pack_params([dict(recs[first], bg=-2)])


def test_c_abi_exports_the_augmentation_entry_points():
    from cosypose_amd.build import build, LIB
    from cosypose_amd import _lib, augmentations as aug
    build()
    lib = ctypes.CDLL(LIB)
    for name in ('cosy_augment_workspace_bytes', 'cosy_augment_batch'):
        assert name in _lib.EXPORTS, name           # test_c_abi.py: EXPORTS, the header and the built library name the same entry points
    f = lib.cosy_augment_workspace_bytes
    f.restype, f.argtypes = ctypes.c_size_t, [ctypes.c_int] * 3
    assert f(64, 480, 640) >= 2 * 64 * 3 * 480 * 640 + 64 * 8 and f(0, 480, 640) == 0
    import cosypose_amd
    assert cosypose_amd.augment_batch is aug.augment_batch and cosypose_amd.draw_sample_params is aug.draw_sample_params
    assert cosypose_amd.pack_params is aug.pack_params


def test_augmentation_kernels_hold_no_fused_multiply_add():
    """Pillow rounds the product and the sum of its blends and of SMOOTH separately; a v_fma_f32 / v_fmac_f32 / v_mad_f32 in the object
    would give other bytes.  kernels_aug.hip is built with contraction off: its float32 arithmetic is v_mul_f32 and v_add_f32 only."""
    from cosypose_amd import build as hipbuild
    hipbuild.build()
    llvm = '/opt/rocm/lib/llvm/bin/'
    with tempfile.TemporaryDirectory() as tmp:
        co, fat = os.path.join(tmp, 'dev.co'), os.path.join(tmp, 'fat.bin')
        subprocess.run([llvm + 'llvm-objcopy', f'--dump-section=.hip_fatbin={fat}', hipbuild._obj('kernels_aug.hip')], check=True)
        subprocess.run([llvm + 'clang-offload-bundler', '--unbundle', '--type=o', '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', f'--input={fat}',
                        f'--output={co}'], check=True)
        asm = subprocess.run([llvm + 'llvm-objdump', '-d', co], capture_output=True, text=True).stdout
    assert 'v_mul_f32' in asm and 'v_add_f32' in asm
    assert not re.findall(r'v_(?:pk_)?(?:fma|fmac|mac|mad)(?:_legacy|_mix)?_f32', asm)
