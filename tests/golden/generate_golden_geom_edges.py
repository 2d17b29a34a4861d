#!/usr/bin/env python3
"""Generate tests/golden/reference_golden_geom_edges.npz: the reference's own geometry, distance and loss functions
(ylabbe/cosypose, mounted read-only at /root/reference) evaluated in FLOAT64 at a few edge cases -- portrait frame and
portrait crop size, points at and behind the z_min clamp, an object centre outside the frame, n_sym < S, several
ground truths in the disentangled loss, ADD-S.  tests/test_geom_dist_kernels.py holds its float64 restatements (the
yardstick of the GPU tests) against these values on the CPU.

Run in the build container only:   python tests/golden/generate_golden_geom_edges.py
The inputs come from edge_inputs() below (seeded, pure numpy: the test regenerates them by importing this file); the
fixture holds the reference's OUTPUTS only.  No reference source is copied: the reference is imported and executed in
place.  Its text is float32 in a few places (`K.float()`, `.to(torch.float)`, `torch.ones(...)`): float64_reference()
redirects those to float64 while the reference runs, so that its own lines evaluate in double.  The one exception is its
compiled scatter_argmin, which takes float32 distances (pybind11 converts): only the chosen INDEX comes from it, and the
cases here are separated by far more than a float32 rounding.
"""
import contextlib
import pathlib
import sys

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
REPO = HERE.parent.parent
OUT = HERE / 'reference_golden_geom_edges.npz'

Z_MIN, LAMB = float(np.float32(0.1)), float(np.float32(1.4))      # the float32 values the kernels receive, widened


def _rot(rs):
    q, r = np.linalg.qr(rs.randn(3, 3))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def _poses(rs, n, z_lo=0.3, z_hi=2.0, xy=0.2):
    T = np.tile(np.eye(4), (n, 1, 1))
    for i in range(n):
        T[i, :3, :3] = _rot(rs)
        z = rs.uniform(z_lo, z_hi)
        T[i, :3, 3] = (rs.uniform(-xy, xy) * z, rs.uniform(-xy, xy) * z, z)
    return T.astype(np.float32)


def edge_inputs():
    """float32 inputs of the fixture's cases (what a kernel would be given); the reference and the restatements widen them"""
    rs = np.random.RandomState(20240)
    d = {}
    # crop geometry: 5 objects of 5-30 cm, 70 points; item 1 partly behind the clamp, item 2 with a point exactly on it,
    # item 3 centred outside the frame
    B, P = 5, 70
    pts = (rs.uniform(-1, 1, (B, P, 3)) * rs.uniform(0.025, 0.15, (B, 1, 3))).astype(np.float32)
    TCO = _poses(rs, B)
    TCO[1, :3, 3] = (0.01, -0.02, 0.12)
    TCO[2, :3, :3] = np.eye(3); TCO[2, :3, 3] = (0.03, 0.02, np.float32(0.1)); pts[2, 0] = 0.0; pts[2, 1] = (0.01, 0.02, -0.05)
    TCO[3, :3, 3] = (0.9, -0.6, 0.8)
    K = np.tile(np.eye(3, dtype=np.float32), (B, 1, 1))
    K[:, 0, 0] = rs.uniform(500, 700, B); K[:, 1, 1] = K[:, 0, 0] * rs.uniform(0.9, 1.1, B)
    K[:, 0, 2] = rs.uniform(230, 250, B); K[:, 1, 2] = rs.uniform(310, 330, B)
    d.update(cg_pts=pts, cg_TCO=TCO, cg_K=K)
    # pose update and the two initialisations
    pose9 = (rs.randn(B, 9) * 0.2 + np.array([1, 0, 0, 0, 1, 0, 0, 0, 1])).astype(np.float32)
    boxes = np.stack([rs.uniform(0, 200, B), rs.uniform(0, 300, B), rs.uniform(250, 470, B), rs.uniform(350, 630, B)], 1).astype(np.float32)
    d.update(pu_pose9=pose9, init_boxes=boxes)
    # symmetric distances: 3 objects, S = 4 rows with 1 / 2 / 4 real ones; T1 = T2 . sym_k^-1 . (small motion)
    n_obj, P2, S = 3, 61, 4
    n_sym = np.array([1, 2, 4], np.int32)
    spts = (rs.uniform(-1, 1, (n_obj, P2, 3)) * rs.uniform(0.03, 0.12, (n_obj, 1, 3))).astype(np.float32)
    sym = np.tile(np.eye(4, dtype=np.float32), (n_obj, S, 1, 1))
    for o in range(n_obj):
        for k in range(1, n_sym[o]):
            a = 2 * np.pi * k / n_sym[o]
            sym[o, k, :3, :3] = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], np.float32)
            sym[o, k, :3, 3] = (rs.randn(3) * 0.002).astype(np.float32)
    Bs = 7
    obj = np.array([0, 1, 2, 2, 1, 2, 0], np.int32)
    ks = np.array([0, 1, 3, 0, 0, 2, 0])
    T2 = _poses(rs, Bs)
    T1 = T2.copy()
    for b in range(Bs):
        m = np.eye(4); m[:3, :3] += 0.02 * rs.randn(3, 3); m[:3, 3] = rs.randn(3) * 0.003
        T1[b] = (T2[b].astype(np.float64) @ np.linalg.inv(sym[obj[b], ks[b]].astype(np.float64)) @ m).astype(np.float32)
    d.update(sd_pts=spts, sd_sym=sym, sd_nsym=n_sym, sd_obj=obj, sd_T1=T1, sd_T2=T2)
    # losses: ground truths T2 . sym_k (S = 4, identity-padded rows are exact duplicates); refiner outputs near identity
    out9 = (rs.randn(Bs, 9) * 0.1 + np.array([1, 0, 0, 0, 1, 0, 0, 0, 1])).astype(np.float32)
    Kc = np.tile(np.array([[600., 0, 160], [0, 640., 120], [0, 0, 1]], np.float32), (Bs, 1, 1))
    Kc[:, 0, 0] *= rs.uniform(0.8, 1.2, Bs).astype(np.float32)
    d.update(ls_out9=out9, ls_K_crop=Kc)
    return d


@contextlib.contextmanager
def float64_reference():
    import torch
    saved = (torch.float, torch.Tensor.float, torch.get_default_dtype())
    torch.float = torch.float64
    torch.Tensor.float = lambda self, *a, **k: self.double()
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.float, torch.Tensor.float = saved[0], saved[1]
        torch.set_default_dtype(saved[2])


def save_npz_reproducible(path, arrays):
    """an .npz np.load reads, byte-identical from run to run: sorted keys, stored uncompressed, a fixed time stamp in every
    zip entry (np.savez stamps the current time)"""
    import io
    import zipfile
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_STORED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main():
    import torch
    sys.dont_write_bytecode = True
    sys.path.insert(0, str(HERE))
    from generate_golden import install_stubs
    install_stubs()
    sys.path.insert(0, str(REPO / 'oracle' / '_ref'))
    import cosypose_cext  # noqa: F401  (the reference imports it at module load)
    from cosypose.lib3d.camera_geometry import project_points_robust, boxes_from_uv, get_K_crop_resize
    from cosypose.lib3d.cropping import deepim_boxes
    from cosypose.lib3d.rotations import compute_rotation_matrix_from_ortho6d
    from cosypose.lib3d import cosypose_ops as cops
    from cosypose.lib3d import symmetric_distances as sdist
    from cosypose.lib3d import distances as dst
    from cosypose.lib3d.rigid_mesh_database import BatchedMeshes

    d = edge_inputs()
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    out = {}
    with float64_reference(), torch.no_grad():
        pts, K, TCO = t(d['cg_pts']), t(d['cg_K']), t(d['cg_TCO'])
        B = len(pts)
        for tag, im_size, crop in (('pp', (640, 480), (320, 240)), ('ll', (480, 640), (240, 320)), ('lp', (480, 640), (320, 240))):
            # the body of PosePredictor.crop_inputs (models/pose.py:45-67) and deepim_crops_robust (cropping.py:64-72) without the pixels
            uv = project_points_robust(pts, K, TCO, z_min=Z_MIN)
            boxes_rend = boxes_from_uv(uv)
            center = project_points_robust(torch.zeros(B, 1, 3), K, TCO, z_min=Z_MIN)
            boxes_crop = deepim_boxes(center, boxes_rend, boxes_rend, im_size=im_size, lamb=LAMB)
            K_crop = get_K_crop_resize(K=K.clone(), boxes=boxes_crop, orig_size=im_size, crop_resize=crop)
            out[f'cg_{tag}_boxes_rend'] = boxes_rend.numpy(); out[f'cg_{tag}_boxes_crop'] = boxes_crop.numpy()
            out[f'cg_{tag}_K_crop'] = K_crop.numpy()
        pose9 = t(d['pu_pose9'])
        dR = compute_rotation_matrix_from_ortho6d(pose9[:, :6])
        out['pu_TCO_out'] = cops.apply_imagespace_predictions(TCO, t(out['cg_ll_K_crop']), pose9[:, 6:9], dR).numpy()
        boxes = t(d['init_boxes'])
        out['init_v0'] = cops.TCO_init_from_boxes(z_range=(0.75, 1.25), boxes=boxes, K=K).numpy()
        out['init_zup'] = cops.TCO_init_from_boxes_zup_autodepth(boxes, pts, K).numpy()

        n_obj = len(d['sd_pts'])
        labels_all = np.array([f'obj_{i:06d}' for i in range(1, n_obj + 1)])
        infos = {l: dict(label=l, n_points=d['sd_pts'].shape[1], n_sym=int(d['sd_nsym'][i])) for i, l in enumerate(labels_all)}
        mesh_db = BatchedMeshes(infos, labels_all, t(d['sd_pts']), t(d['sd_sym'])).float()
        labels = labels_all[d['sd_obj']]
        T1, T2 = t(d['sd_T1']), t(d['sd_T2'])
        d0, S0 = sdist.symmetric_distance_batched(T1, T2, labels, mesh_db)
        d1, S1 = sdist.symmetric_distance_batched_fast(T1, T2, labels, mesh_db)
        out.update(sd_batched_dists=d0.numpy(), sd_batched_S12=S0.numpy(), sd_fast_dists=d1.numpy(), sd_fast_S12=S1.numpy())
        points = t(d['sd_pts'][d['sd_obj']])
        gt = T2.unsqueeze(1) @ t(d['sd_sym'][d['sd_obj']])
        loss, assign = cops.loss_CO_symmetric(gt, T1, points)
        out.update(ls_loss=loss.numpy(), ls_assign=assign.numpy())
        out['ls_disentangled'] = cops.loss_refiner_CO_disentangled(gt, T1, t(d['ls_out9']), t(d['ls_K_crop']), points).numpy()
        out['add'] = dst.dists_add(T1, T2, points).numpy()
        out['adds'] = dst.dists_add_symmetric(T1, T2, points).numpy()
    for k, v in out.items():
        assert v.dtype == np.float64, (k, v.dtype)
    save_npz_reproducible(OUT, out)
    print('wrote', OUT, OUT.stat().st_size, 'bytes')


if __name__ == '__main__':
    main()
