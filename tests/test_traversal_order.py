"""The order in which a backbone launch walks the samples (cosy_effnet_b3_set_traversal; csrc/job_order.h, effnet.hip: plan_traversal).

Mode 0: every launch walks the batch forward.  Mode 1 (serpentine): a launch that reads a large activation walks it in the opposite order to
the launch that wrote it.  A job's arithmetic does not depend on when it runs and the squeeze sums are reduced per band in a fixed order, so the
two modes must agree BIT FOR BIT on every tensor: pose, features, the depthwise output D of every block (probe 100 + i) and every block output
(probe i).  A reversed decode that drops, doubles or mis-assigns a job leaves part of a tensor stale or wrong, which torch.equal sees.

The decode itself (job_order.h is plain C++ as well) is checked on the CPU by a stand-alone program: a bijection that keeps the XCD residue.
"""
import ctypes
import pathlib
import subprocess

import numpy as np
import pytest
import torch

REPO = pathlib.Path(__file__).resolve().parent.parent
EINVAL = -1      # include/cosyhip.h: COSY_EINVAL


@pytest.fixture(scope='module')
def model(golden_sd):
    import argparse
    from cosypose_amd import synthetic as syn
    from cosypose_amd.pose_models_cfg import create_model_pose, check_update_config
    from cosypose_amd.mesh_db import BatchedMeshes
    labels = np.array([f'obj_{i:06d}' for i in range(1, 4)])
    infos = {l: dict(label=l, n_points=500, n_sym=1) for l in labels}
    mesh_db = BatchedMeshes(infos, labels, torch.from_numpy(syn.make_mesh_points(7, 3, 500)), torch.eye(4).reshape(1, 1, 4, 4).repeat(3, 1, 1, 1)).float().cuda()
    cfg = check_update_config(argparse.Namespace(backbone_str='efficientnet-b3', n_pose_dims=9))
    m = create_model_pose(cfg, None, mesh_db)      # (the backbone alone is run: no renderer)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in golden_sd.items()}, strict=False)
    return m.cuda().eval()


def _engine(model, hw, dtype, B):
    from cosypose_amd._lib import lib, check
    model.compute_dtype = dtype
    model.render_size = tuple(hw)
    h = model._net(B, torch.device('cuda'))
    plan = []
    for i in range(26):
        dims = (ctypes.c_int * 11)()
        check(lib().cosy_effnet_b3_block_info(h, i, dims))
        plan.append(list(dims))
    return h, plan


def _forward(h, B, mode, layer=-2, shape=None):
    """one forward in `mode`; -> (pose, features, the probed activation `layer` as fp32 NCHW or None), all on the device"""
    from cosypose_amd._lib import lib, check, ptr, stream
    pose = torch.empty(B, 9, device='cuda'); feat = torch.empty(B, 1536, device='cuda')
    out = torch.empty(shape, device='cuda') if shape else None
    check(lib().cosy_effnet_b3_set_traversal(h, mode))
    check(lib().cosy_effnet_b3_set_probe(h, layer, ptr(out)))
    try:
        check(lib().cosy_effnet_b3_forward(h, B, ptr(feat), ptr(pose), None, stream()))
        torch.cuda.synchronize()
    finally:
        check(lib().cosy_effnet_b3_set_probe(h, -2, None))
    return pose, feat, out


# crop size, storage type, batch: what the case reaches
CASES = [
    ((256, 256), 'fp16', 1),      # fewer samples than XCDs: most workgroups of a reversed grid return early, and they come FIRST
    ((256, 256), 'fp16', 3),      # the size of the storage-emulation test
    ((256, 256), 'fp16', 9),      # one sample beyond a full round of the eight XCDs: a ragged last round, an odd last pair for the two-sample 8x8-map front
    ((256, 256), 'bf16', 3),      # hi + lo weight pairs; blocks 19-25 unfused (expand GEMM -> depthwise kernel -> project GEMM)
    ((240, 320), 'fp16', 3),      # transposed walks, column-major stages, the re-ordering copy behind them, the 7x10-map front
    ((224, 224), 'fp16', 3),      # tiled front, !FULLW wave variants, generic unfused blocks
    ((256, 256), 'fp32', 3),      # the fp32 wave variants and the tiled front on block 2
]


@pytest.mark.gpu
@pytest.mark.parametrize('hw,dtype,B', CASES, ids=['%dx%d-%s-B%d' % (hw + (dt, B)) for hw, dt, B in CASES])
def test_serpentine_order_is_bit_identical(model, hw, dtype, B):
    from cosypose_amd._lib import lib, check, ptr, stream
    x = torch.from_numpy(np.random.RandomState(70 + hw[0] + B).random_sample((B, 6) + tuple(hw)).astype(np.float32)).cuda()
    h, plan = _engine(model, hw, dtype, B)
    try:
        check(lib().cosy_effnet_b3_set_input_nchw(h, ptr(x), B, stream()))
        pose0, feat0, _ = _forward(h, B, 0)
        pose1, feat1, _ = _forward(h, B, 1)
        assert torch.isfinite(pose0).all() and torch.isfinite(feat0).all()
        assert torch.equal(pose0, pose1) and torch.equal(feat0, feat1)
        bad = []
        for i, (H_, W_, Ho, Wo, cin, cmid, cout, *_rest) in enumerate(plan):
            for tag, layer, shape in ((f'D{i}', 100 + i, (B, cmid, Ho, Wo)), (f'y{i}', i, (B, cout, Ho, Wo))):
                p0, f0, a0 = _forward(h, B, 0, layer, shape)
                p1, f1, a1 = _forward(h, B, 1, layer, shape)
                # (every forward of the loop is also a forward after a switch of modes on the same engine: nothing of the other mode may linger)
                if not (torch.equal(a0, a1) and torch.equal(p0, pose0) and torch.equal(p1, pose0) and torch.equal(f0, feat0) and torch.equal(f1, feat0)):
                    bad.append((tag, int((a0 != a1).sum()), a0.numel()))
        assert not bad, bad
    finally:
        model.compute_dtype = 'fp32'; model.render_size = (240, 320)


@pytest.mark.gpu
def test_set_traversal_rejects_other_modes(model):
    from cosypose_amd._lib import lib, check, ptr, stream
    B = 2
    h, _ = _engine(model, (256, 256), 'fp16', B)
    try:
        x = torch.from_numpy(np.random.RandomState(5).random_sample((B, 6, 256, 256)).astype(np.float32)).cuda()
        check(lib().cosy_effnet_b3_set_input_nchw(h, ptr(x), B, stream()))
        pose1, feat1, _ = _forward(h, B, 1)
        for mode in (-1, 2, 3, 1 << 20):
            assert lib().cosy_effnet_b3_set_traversal(h, mode) == EINVAL
            assert b'set_traversal' in lib().cosy_last_error()
        assert lib().cosy_effnet_b3_set_traversal(None, 0) == EINVAL
        # a refused mode leaves the engine as it was: still mode 1, the same bits; and mode 0 after it as well
        pose = torch.empty(B, 9, device='cuda'); feat = torch.empty(B, 1536, device='cuda')
        check(lib().cosy_effnet_b3_forward(h, B, ptr(feat), ptr(pose), None, stream()))
        torch.cuda.synchronize()
        assert torch.equal(pose, pose1) and torch.equal(feat, feat1)
        pose0, feat0, _ = _forward(h, B, 0)
        assert torch.equal(pose0, pose1) and torch.equal(feat0, feat1)
    finally:
        model.compute_dtype = 'fp32'; model.render_size = (240, 320)


DECODE_PROGRAM = r'''
#include <cstdio>
#include <set>
#include <utility>
#include "job_order.h"
int main() {
    for (unsigned grid = 8; grid <= 8 * 41; grid += 8) {
        std::set<std::pair<int, int>> fwd, rev;
        for (unsigned id = 0; id < grid; ++id) {
            const cosy::JobId f = cosy::job_decode(id, grid, 0), r = cosy::job_decode(id, grid, 1);
            if (f.xcd != (int)(id & 7) || f.jj != (int)(id >> 3)) { printf("forward decode of %u / %u\n", id, grid); return 1; }
            if (r.xcd != (int)(id & 7)) { printf("XCD residue of %u / %u\n", id, grid); return 1; }
            if (r.jj != (int)(grid >> 3) - 1 - (int)(id >> 3)) { printf("reversed job of %u / %u\n", id, grid); return 1; }
            if (r.jj < 0 || r.jj >= (int)(grid >> 3)) { printf("range of %u / %u\n", id, grid); return 1; }
            fwd.insert({f.xcd, f.jj}); rev.insert({r.xcd, r.jj});
        }
        if (fwd.size() != grid || rev != fwd) { printf("not a bijection at grid %u\n", grid); return 1; }
    }
    for (unsigned grid = 1; grid <= 333; ++grid) {      // the plain grids: any size
        std::set<int> seen;
        for (unsigned id = 0; id < grid; ++id) {
            if (cosy::job_linear(id, grid, 0) != (int)id) { printf("forward linear %u / %u\n", id, grid); return 1; }
            seen.insert(cosy::job_linear(id, grid, 1));
        }
        if (seen.size() != grid || *seen.begin() != 0 || *seen.rbegin() != (int)grid - 1) { printf("linear not a bijection at grid %u\n", grid); return 1; }
    }
    printf("ok\n");
    return 0;
}
'''


def test_job_decode_is_a_bijection_that_keeps_the_xcd(tmp_path):
    """csrc/job_order.h under the host C++ compiler: for grids of 8 ... 8 * 41 workgroups the reversed decode visits every (xcd, jj) exactly once and
    keeps id & 7; the mirrored plain id is a permutation for every grid size"""
    (tmp_path / 'decode.cpp').write_text(DECODE_PROGRAM)
    cc = subprocess.run(['g++', '-std=c++17', '-Wall', '-Werror', '-I', str(REPO / 'cosypose_amd' / 'csrc'), str(tmp_path / 'decode.cpp'), '-o', str(tmp_path / 'decode')],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    run = subprocess.run([str(tmp_path / 'decode')], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == 'ok', run.stdout[-2000:]
