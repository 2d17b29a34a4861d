"""ADD / ADD-S point distances, same surface as the reference's cosypose/lib3d/distances.py:5-21
(HIP: cosy_dists_add; the (B,P,P,3) intermediate of dists_add_symmetric never exists)."""
import torch

from ._lib import lib, check, ptr, stream, require_device


def _dists(TXO_pred, TXO_gt, points, symmetric):
    bsz, n_pts = points.shape[:2]
    assert TXO_pred.shape == (bsz, 4, 4) and TXO_gt.shape == (bsz, 4, 4) and points.shape == (bsz, n_pts, 3)
    out = torch.empty(bsz, n_pts, 3, device=points.device)
    if bsz == 0:
        return out
    require_device(TXO_pred, TXO_gt, points)
    p, g, pts = (t.detach().float().contiguous() for t in (TXO_pred, TXO_gt, points))
    check(lib().cosy_dists_add(ptr(p), ptr(g), ptr(pts), None, bsz, n_pts, int(symmetric), ptr(out), stream()))
    return out


def dists_add(TXO_pred, TXO_gt, points):
    """gt points - predicted points, (B,P,3)"""
    return _dists(TXO_pred, TXO_gt, points, False)


def dists_add_symmetric(TXO_pred, TXO_gt, points):
    """every gt point minus its NEAREST predicted point, (B,P,3)"""
    return _dists(TXO_pred, TXO_gt, points, True)


def pose_errors(TXO_pred, TXO_gt, obj_ids, modes, pts_table, n_points):
    """PoseErrorMeter.compute_errors (cosypose/evaluation/meters/pose_meters.py:53-92) for B tentative pairs in one launch
    (HIP: cosy_pose_errors), each on pts_table[obj_ids[b], :n_points[obj_ids[b]]] with its own mode (0 = ADD, 1 = ADD-S).
    -> dict(norm_avg (B), xyz_avg (B,3), TCO_xyz (B,3), TCO_norm (B)) of fp32 device tensors."""
    from ._lib import ints_to_device
    bsz = TXO_pred.shape[0]
    assert TXO_pred.shape == (bsz, 4, 4) and TXO_gt.shape == (bsz, 4, 4) and pts_table.dim() == 3 and pts_table.shape[2] == 3
    n_obj, n_max = pts_table.shape[:2]
    require_device(TXO_pred, TXO_gt, pts_table)
    dev = pts_table.device
    out = torch.empty(bsz, 8, device=dev)
    if bsz > 0:
        p, g, pts = (t.detach().float().contiguous() for t in (TXO_pred, TXO_gt, pts_table))
        obj, mode, n_pts = (ints_to_device(v, dev) for v in (obj_ids, modes, n_points))
        assert obj.shape == (bsz,) and mode.shape == (bsz,) and n_pts.shape == (n_obj,)
        ws_bytes = lib().cosy_pose_errors_workspace_bytes(bsz, n_max)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        check(lib().cosy_pose_errors(ptr(p), ptr(g), ptr(obj), ptr(mode), ptr(pts), ptr(n_pts), bsz, n_obj, n_max, ptr(out), ptr(ws),
                                     ws_bytes, stream()))
    return dict(norm_avg=out[:, 0], xyz_avg=out[:, 1:4], TCO_xyz=out[:, 4:7], TCO_norm=out[:, 7])
