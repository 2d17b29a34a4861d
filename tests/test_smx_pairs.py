"""mbconv_small_mx_kernel with two samples per workgroup (kernels_smx.hip, SPW = 2: the fp16 fronts of blocks 19-25 on the 8x8 maps).

CPU: the form pays only while two of its 8-wave workgroups share a CU (16 waves, 4 per SIMD): <= 128 VGPRs, no scratch, no AGPR split, <= 80 KB of LDS.
Block 25's instantiation (k = 3, 12 k-blocks) sits exactly on the register cliff; one more register halves the occupancy without failing anything else.

GPU: a sample's D, squeeze-excite gate and block output must not depend on the sample it shares a workgroup with, on its place in the batch or on the
missing partner of an odd batch's last sample: whole tensors, bit for bit, against the same sample run alone."""
import os
import re
import shutil

import numpy as np
import pytest

needs_hipcc = pytest.mark.skipif(shutil.which('hipcc') is None and not os.path.exists('/opt/rocm/bin/hipcc'), reason='needs hipcc')

NETWORK_SHAPES = {(3, 8), (3, 12), (5, 8)}      # (k, k-blocks of Cin) of blocks 24, 25 and 19-23


def _lds_bytes(ks, kbn, nseg, spw):
    """the launcher's dynamic LDS (kernels_smx.hip: smx_lds_bytes, fp16): per sample the E operands [nseg + 2][3][64] x 8 bytes and the squeeze partials
    [nseg][48] fp32; once the weight ring [3][kbn] x 1 KB and two parameter buffers (1 KB header + [3][ks][2] x 512 bytes of Toeplitz fragments)"""
    return spw * (nseg + 2) * 3 * 512 + 3 * kbn * 1024 + 2 * (1024 + 3 * ks * 2 * 512) + spw * nseg * 48 * 4


@needs_hipcc
def test_pair_instantiations_keep_four_waves_per_simd():
    from cosypose_amd import build
    build.build()
    res = build.kernel_resources(demangle=False)      # Itanium names: ...mbconv_small_mx_kernelI<T>Li<KS>ELi<KBN>ELi<NSEG>ELi<SPW>EEE...
    pat = re.compile(r'mbconv_small_mx_kernelI(DF16_|DF16b)Li(\d+)ELi(\d+)ELi(\d+)ELi(\d+)EEE')
    pairs = {}
    for name, r in res.items():
        m = pat.search(name)
        assert m or 'mbconv_small_mx_kernel' not in name, name
        if m and int(m.group(5)) == 2:
            assert m.group(1) == 'DF16_' and int(m.group(4)) == 4, name      # fp16, 8x8 maps only
            pairs[(int(m.group(2)), int(m.group(3)))] = r
    assert set(pairs) == NETWORK_SHAPES, sorted(pairs)
    for (ks, kbn), r in pairs.items():
        print(f'SPW=2 k{ks} kbn{kbn}: {r}, dynamic LDS {_lds_bytes(ks, kbn, 4, 2)}')
        assert r['scratch'] == 0 and r['agpr'] == 0 and r['vgpr'] <= 128 and r['occupancy'] >= 4, ((ks, kbn), r)
        assert r['lds'] == 0 and _lds_bytes(ks, kbn, 4, 2) <= 80 * 1024, (ks, kbn)      # (the source holds the launcher's own figure to the same bound: static_assert)


def test_kernel_name_carries_every_template_argument():
    """the name the schedule reports (event tables, roofline, PMC prefix) is the instantiation as the profiler prints it, and bench.py's
    issue-slot model still reads k from its third field"""
    import importlib.util
    from conftest import REPO
    src = open(REPO / 'cosypose_amd' / 'csrc' / 'kernels_smx.hip').read()
    assert '"mbconv_small_mx_kernel<%s, %d, %d, %d, %d>"' in src
    assert re.search(r'template <typename T, int KS, int KBN, int NSEG, int SPW>\s*\n__global__', src)
    spec = importlib.util.spec_from_file_location('bench_for_names', REPO / 'bench.py')
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    k = dict(layers=[19, 20, 21, 22, 23], ms=0.25, n=5)
    vb = bench.valu_bound('mbconv_small_mx_kernel<_Float16, 5, 8, 4, 2>', k, 256, (256, 256), {l: 6 for l in k['layers']})
    old = bench.valu_bound('mbconv_small_mx_kernel<_Float16, 5, 8>', k, 256, (256, 256), {l: 6 for l in k['layers']})
    assert vb is not None and vb == old and vb['taps'] == 'matrix pipe'


# ---------------------------------------------------------------------------------------------
# GPU: pairing, odd tails and position change nothing
# ---------------------------------------------------------------------------------------------
HW = (256, 256)
BLOCKS = range(19, 26)
N_BASE = 4


def _base_samples():
    return np.random.RandomState(1925).random_sample((N_BASE, 6) + HW).astype(np.float32)


def _run(model, x):
    """{(tag, block): whole fp32 tensor} of D (probe 100 + i), gate (200 + i) and output (probe i) of blocks 19-25 for the batch x"""
    from test_gpu_parity import _block_plan, _probe, dev
    from cosypose_amd._lib import lib, check, ptr, stream
    B = x.shape[0]
    h, plan = _block_plan(model, HW, 'fp16', B)
    assert all(plan[i][7] == 6 and plan[i][0] == 8 and plan[i][1] == 8 for i in BLOCKS), [p[7] for p in plan]      # the matrix-pipe 8x8-map front
    check(lib().cosy_effnet_b3_set_input_nchw(h, ptr(dev(x)), B, stream()))
    out = {}
    for i in BLOCKS:
        _, _, Ho, Wo, _, cmid, cout = plan[i][:7]
        out['D', i] = _probe(model, h, x, 100 + i, (B, cmid, Ho, Wo))
        out['g', i] = _probe(model, h, x, 200 + i, (B, cmid))
        out['y', i] = _probe(model, h, x, i, (B, cout, Ho, Wo))
    return out


@pytest.fixture(scope='module')
def model(golden_sd):
    import argparse
    import torch
    from cosypose_amd import synthetic as syn
    from cosypose_amd.pose_models_cfg import create_model_pose, check_update_config
    from cosypose_amd.mesh_db import BatchedMeshes
    labels = np.array([f'obj_{i:06d}' for i in range(1, 22)])
    mesh_db = BatchedMeshes({l: dict(label=l, n_points=2500, n_sym=1) for l in labels}, labels, torch.from_numpy(syn.make_mesh_points(7, 21, 2500)),
                            torch.eye(4).reshape(1, 1, 4, 4).repeat(21, 1, 1, 1)).float().cuda()
    cfg = check_update_config(argparse.Namespace(backbone_str='efficientnet-b3', n_pose_dims=9))
    m = create_model_pose(cfg, None, mesh_db)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in golden_sd.items()}, strict=False)
    m.cfg = cfg
    return m.cuda().eval()


@pytest.fixture(scope='module')
def alone(model):
    """every base sample run alone (B = 1)"""
    xs = _base_samples()
    return [_run(model, xs[j:j + 1]) for j in range(N_BASE)]


@pytest.mark.gpu
@pytest.mark.parametrize('B', [1, 2, 3, 17, 64])
def test_sample_values_do_not_depend_on_partner_position_or_tail(model, alone, B):
    """Batch row j holds base sample (j + shift) % 4, for shift 0 and 1: every base sample sits at even and at odd rows (first and second sample of a
    pair, next to different partners) and, for odd B, alone in the last pair.  Each row of D, gate and output of blocks 19-25 must equal, bit for bit,
    what the same sample gives at B = 1 -- hence also what it gives at any other row."""
    xs = _base_samples()
    bad = []
    try:
        for shift in (0, 1):
            idx = [(j + shift) % N_BASE for j in range(B)]
            got = _run(model, xs[idx])
            for key, t in got.items():
                assert np.isfinite(t).all(), key
                for j, src in enumerate(idx):
                    if not np.array_equal(t[j], alone[src][key][0]):
                        bad.append((key, B, shift, j, float(np.abs(t[j] - alone[src][key][0]).max())))
    finally:
        model.compute_dtype = 'fp32'; model.render_size = (240, 320)
    assert not bad, bad[:10]
