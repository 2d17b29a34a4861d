"""BOP pose errors on the device: MSSD, MSPD and VSD (Hodan et al., "BOP Challenge 2020", section 2.2) of B tentative
(estimate, ground truth) pairs in one call.  HIP: csrc/kernels_bop.hip behind cosy_bop_mssd_mspd, cosy_bop_instance_boxes,
cosy_bop_render_windows and cosy_bop_vsd_counts; DESIGN.md section 15 holds the contract and the arithmetic, tests/bop_ref.py its
numpy twins.

The reference does not compute these numbers itself: scripts/run_bop_eval.py:58-70 writes a CSV and starts the BOP toolkit, which
renders every estimate on the CPU.  Here every distinct (object, view, pose) is rendered once into a window the size of its own pixel
box, and a pair compares two windows with the measured depth.
"""
import inspect
import sys
import types

import numpy as np
import torch

from ._lib import lib, check, ptr, stream, require_device, ints_to_device, host_to_device
from .rasterizer import RenderMeshes

VSD_DELTA = 0.015                                                    # visibility tolerance, metres
VSD_TAUS = tuple(round(0.05 * k, 2) for k in range(1, 11))           # misalignment tolerances, times the object's diameter
VSD_THRESHOLDS = tuple(round(0.05 * k, 2) for k in range(1, 11))     # thresholds of correctness on e_vsd
MSSD_THRESHOLDS = tuple(round(0.05 * k, 2) for k in range(1, 11))    # times the object's diameter
MSPD_THRESHOLDS = tuple(float(5 * k) for k in range(1, 11))          # pixels, times (image width / 640)
MAX_TAUS = 16


class BopModels:
    """The object set of the BOP errors: RenderMeshes (`meshes`) plus, per label, the number of vertices n_verts (the padded rows of
    the vertex table are not part of the object), the symmetry table sym_table (n_obj,S,4,4) with n_sym used rows -- the identity
    first -- and the diameter in metres.  symmetries: one (n,4,4) array per label, or None (identity only); diameters: one per label,
    or None: the diagonal of the vertices' bounding box."""

    def __init__(self, labels, verts_list, faces_list, symmetries=None, diameters=None, colors_list=None):
        self.meshes = RenderMeshes(labels, verts_list, faces_list, colors_list)
        self.labels, self.label_to_id = self.meshes.labels, self.meshes.label_to_id
        n = len(labels)
        syms = [np.eye(4)[None] if symmetries is None or symmetries[i] is None else np.asarray(symmetries[i], np.float64).reshape(-1, 4, 4)
                for i in range(n)]
        S = max(len(s) for s in syms)
        table = np.tile(np.eye(4, dtype=np.float32), (n, S, 1, 1))
        for i, s in enumerate(syms):
            assert len(s) >= 1 and np.array_equal(s[0], np.eye(4)), 'the identity comes first in every symmetry list'
            table[i, :len(s)] = s
        self.sym_table = torch.from_numpy(table)
        self.n_sym = torch.tensor([len(s) for s in syms], dtype=torch.int32)
        self.n_verts = torch.tensor([len(v) for v in verts_list], dtype=torch.int32)
        if diameters is None:
            diameters = [float(np.linalg.norm(np.asarray(v, np.float64).max(0) - np.asarray(v, np.float64).min(0))) for v in verts_list]
        self.diameters = np.asarray(diameters, dtype=np.float64)
        assert self.diameters.shape == (n,)

    @classmethod
    def from_mesh_db(cls, mesh_db, verts_list, faces_list, colors_list=None):
        """symmetries and diameters from a BatchedMeshes: its `symmetries` (n_obj,S,4,4) and, per label, infos['n_sym'] (all S rows when
        absent) and infos['diameter_m']; verts_list / faces_list in the order of mesh_db.labels."""
        labels = list(mesh_db.labels)
        sym = mesh_db.symmetries.detach().cpu().numpy()
        infos = mesh_db.infos
        syms = [sym[i, :int(infos[l].get('n_sym', sym.shape[1]))] for i, l in enumerate(labels)]
        return cls(labels, verts_list, faces_list, symmetries=syms, diameters=[infos[l]['diameter_m'] for l in labels], colors_list=colors_list)

    def cuda(self):
        self.meshes.cuda()
        for k in ('sym_table', 'n_sym', 'n_verts'):
            setattr(self, k, getattr(self, k).cuda().contiguous())
        return self


def vsd_from_counts(counts):
    """e_k = (c_k + |U| - |I|) / |U| in float64, 1 where |U| = 0; counts (..., 2 + n_tau) integers (numpy array or tensor)"""
    if isinstance(counts, torch.Tensor):
        c = counts.to(torch.float64)
        u, i = c[..., 0:1], c[..., 1:2]
        return torch.where(u > 0, (c[..., 2:] + u - i) / u.clamp(min=1.0), torch.ones_like(c[..., 2:]))
    c = np.asarray(counts, dtype=np.float64)
    u, i = c[..., 0:1], c[..., 1:2]
    return np.where(u > 0, (c[..., 2:] + u - i) / np.maximum(u, 1.0), 1.0)


def absolute_taus(taus, obj_ids, diameters):
    """(B, n_tau) float32 metres: taus (n_tau,) are fractions of each pair's object diameter (the product is formed in float64 and
    rounded once); a (B, n_tau) array is taken as metres already."""
    taus = np.asarray(taus, dtype=np.float64)
    if taus.ndim == 1:
        taus = taus[None, :] * np.asarray(diameters, np.float64)[np.asarray(obj_ids, dtype=np.int64)][:, None]
    assert taus.ndim == 2 and taus.shape[0] == len(obj_ids) and 1 <= taus.shape[1] <= MAX_TAUS, taus.shape
    return np.ascontiguousarray(taus.astype(np.float32))


def plan_windows(boxes, est_inst, gt_inst, max_pixels=None):
    """The host half of the depth windows, no device needed.  boxes (N,4) int x0, y0, x1, y1 inclusive (empty: x1 < x0 or y1 < y0),
    est_inst / gt_inst (B,) the instances of every pair, max_pixels the cap of the window store or None.
    -> list of chunks dict(lo, hi, win_offset (N,) int64, n_pixels): pairs [lo, hi) are compared while the windows of exactly their
    instances are in the store (win_offset = -1: not in this chunk).  Pairs stay in order; an instance that two chunks need is
    rendered in both.  A single pair whose two windows exceed the cap is refused."""
    boxes = np.asarray(boxes, dtype=np.int64).reshape(-1, 4)
    size = np.maximum(boxes[:, 2] - boxes[:, 0] + 1, 0) * np.maximum(boxes[:, 3] - boxes[:, 1] + 1, 0)
    est_inst, gt_inst = np.asarray(est_inst, dtype=np.int64), np.asarray(gt_inst, dtype=np.int64)
    B, N = len(est_inst), len(boxes)

    def chunk(lo, hi):
        used = np.unique(np.concatenate([est_inst[lo:hi], gt_inst[lo:hi]]))
        used = used[size[used] > 0]
        off = np.full(N, -1, dtype=np.int64)
        off[used] = np.cumsum(size[used]) - size[used]
        return dict(lo=lo, hi=hi, win_offset=off, n_pixels=int(size[used].sum()))

    if B == 0:
        return []
    if max_pixels is None or chunk(0, B)['n_pixels'] <= max_pixels:
        return [chunk(0, B)]
    chunks, lo, have, total = [], 0, set(), 0
    for b in range(B):
        new = {int(est_inst[b]), int(gt_inst[b])} - have
        add = int(sum(size[n] for n in new))
        if total + add > max_pixels and b > lo:
            chunks.append(chunk(lo, b))
            lo, have, total = b, set(), 0
            new = {int(est_inst[b]), int(gt_inst[b])}
            add = int(sum(size[n] for n in new))
        if add > max_pixels:
            raise ValueError(f'max_workspace_bytes holds {max_pixels} window pixels; pair {b} alone needs {add}')
        have |= new
        total += add
    chunks.append(chunk(lo, B))
    return chunks


def instance_boxes(TCO, obj_ids, view_ids, K, models, resolution):
    """(N,4) int32 device tensor: the pixel box x0, y0, x1, y1 (inclusive, clipped to the frame) of every instance; empty boxes have
    x1 < x0 or y1 < y0, and x1 = y1 = -2 marks an instance that cannot be drawn at all (a non-finite pose or K, ids outside the tables):
    its pairs get zero counts"""
    m = models.meshes
    N, (H, W) = len(TCO), resolution
    boxes = torch.empty(N, 4, dtype=torch.int32, device=TCO.device)
    check(lib().cosy_bop_instance_boxes(ptr(TCO), ptr(obj_ids), ptr(view_ids), ptr(K), ptr(m.verts), ptr(models.n_verts), N, m.verts.shape[0],
                                        len(K), m.verts.shape[1], H, W, ptr(boxes), stream()))
    return boxes


def render_windows(TCO, obj_ids, view_ids, K, models, resolution, boxes, win_offset, n_pixels, store=None):
    """the packed depth windows (n_pixels,) float32 of the instances whose win_offset is >= 0"""
    m = models.meshes
    N, (H, W) = len(TCO), resolution
    need = lib().cosy_bop_windows_workspace_bytes(n_pixels)
    if store is None or store.numel() * 4 < need:
        store = torch.empty(max(need // 4, 4), dtype=torch.float32, device=TCO.device)
    check(lib().cosy_bop_render_windows(ptr(TCO), ptr(obj_ids), ptr(view_ids), ptr(K), ptr(m.verts), ptr(m.faces), ptr(m.n_faces), ptr(boxes),
                                        ptr(win_offset), N, m.verts.shape[0], len(K), m.verts.shape[1], m.faces.shape[1], H, W, n_pixels,
                                        ptr(store), store.numel() * 4, stream()))
    return store


def mssd_mspd(TCO_pred, TCO_gt, obj_ids, view_ids, K, models):
    """-> (mssd (B,), mspd (B,)) float32 device tensors; ids are int32 device tensors"""
    m = models.meshes
    B, dev = len(TCO_pred), TCO_pred.device
    out = torch.empty(2, B, device=dev)
    if B:
        S = models.sym_table.shape[1]
        ws_bytes = lib().cosy_bop_mssd_mspd_workspace_bytes(B, S)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        check(lib().cosy_bop_mssd_mspd(ptr(TCO_pred), ptr(TCO_gt), ptr(obj_ids), ptr(view_ids), ptr(K), ptr(m.verts), ptr(models.n_verts),
                                       ptr(models.sym_table), ptr(models.n_sym), B, m.verts.shape[0], len(K), m.verts.shape[1], S, ptr(out[0]),
                                       ptr(out[1]), ptr(ws), ws_bytes, stream()))
    return out[0], out[1]


def unique_instances(TCO_pred, TCO_gt, obj_ids, view_ids):
    """Every distinct (pose bits, object, view) among the 2 B estimates and ground truths once.
    -> (TCO (N,4,4), obj (N,), view (N,), est_inst (B,), gt_inst (B,)) device tensors"""
    B = len(TCO_pred)
    ids = torch.stack([obj_ids, view_ids], 1).repeat(2, 1)
    rows = torch.cat([torch.cat([TCO_pred, TCO_gt]).reshape(2 * B, 16).view(torch.int32), ids], 1)
    uniq, inverse = torch.unique(rows, dim=0, return_inverse=True)
    TCO = uniq[:, :16].contiguous().view(torch.float32).reshape(-1, 4, 4)
    inverse = inverse.to(torch.int32)
    return TCO, uniq[:, 16].contiguous(), uniq[:, 17].contiguous(), inverse[:B].contiguous(), inverse[B:].contiguous()


def vsd_counts(TCO_pred, TCO_gt, obj_ids, view_ids, K, depth, models, taus_abs, delta=VSD_DELTA, max_workspace_bytes=None, timings=None):
    """counts (B, 2 + n_tau) int32 on the device.  ids: int32 device tensors, taus_abs (B, n_tau) float32 device tensor.  The host waits
    for the device twice: torch.unique sizes its output, and the boxes come back together with the pairs' instance numbers in ONE
    device -> host copy, to size the windows."""
    B, dev = len(TCO_pred), TCO_pred.device
    n_tau = taus_abs.shape[1]
    counts = torch.zeros(B, 2 + n_tau, dtype=torch.int32, device=dev)
    if B == 0:
        return counts
    H, W = depth.shape[1:]
    mark = (lambda: None) if timings is None else (lambda: timings.append(_event()))
    mark()
    TCO, obj, view, est_inst, gt_inst = unique_instances(TCO_pred, TCO_gt, obj_ids, view_ids)
    boxes = instance_boxes(TCO, obj, view, K, models, (H, W))
    cap = None if max_workspace_bytes is None else int(max_workspace_bytes) // 4
    host = torch.cat([boxes.reshape(-1), est_inst, gt_inst]).cpu().numpy()          # one copy: boxes (N,4) | est_inst (B) | gt_inst (B)
    chunks = plan_windows(host[:4 * len(TCO)].reshape(-1, 4), host[4 * len(TCO):4 * len(TCO) + B], host[4 * len(TCO) + B:], cap)
    ws_bytes = lib().cosy_bop_vsd_workspace_bytes(B)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    store = None
    for c in chunks:
        lo, hi = c['lo'], c['hi']
        off = host_to_device(c['win_offset'], dev)
        store = render_windows(TCO, obj, view, K, models, (H, W), boxes, off, c['n_pixels'], store)
        mark()
        check(lib().cosy_bop_vsd_counts(ptr(est_inst[lo:hi]), ptr(gt_inst[lo:hi]), ptr(view), ptr(boxes), ptr(off), ptr(store), c['n_pixels'],
                                        ptr(depth), ptr(K), ptr(taus_abs[lo:hi]), float(delta), hi - lo, len(TCO), len(K), n_tau, H, W,
                                        ptr(counts[lo:hi]), ptr(ws), ws_bytes, stream()))
        mark()
    return counts


def _event():
    e = torch.cuda.Event(enable_timing=True)
    e.record()
    return e


def bop_errors(TCO_pred, TCO_gt, obj_ids, view_ids, K, depth, models, taus=VSD_TAUS, delta=VSD_DELTA, max_workspace_bytes=None):
    """B pairs: TCO_pred / TCO_gt (B,4,4) device tensors, obj_ids (B,) rows of `models`, view_ids (B,) rows of K (n_views,3,3) and of
    depth (n_views,H,W) float32 metres, 0 = missing; the ids are host values (a device tensor is read back: they are checked here
    and the taus are formed from them on the host).  taus: fractions of the object's diameter (n_tau <= 16), or
    (B, n_tau) metres; delta metres; max_workspace_bytes caps the store of the depth windows (the pairs are then worked off in chunks).
    Ids outside their tables are refused here.
    -> dict: mssd (B,) metres and mspd (B,) pixels, float32; vsd_counts (B, 2 + n_tau) int32 = |U|, |I|, c_k; vsd (B, n_tau) float64
    = (c_k + |U| - |I|) / |U|, 1 where |U| = 0.  Device tensors.  A pair with a non-finite entry in a pose or in its view's K has NaN
    mssd / mspd, zero counts and vsd 1."""
    m = models.meshes
    require_device(m.verts, TCO_pred, TCO_gt, K, depth)
    TCO_pred, TCO_gt, K = (torch.as_tensor(t).detach().float().contiguous() for t in (TCO_pred, TCO_gt, K))
    B, dev = len(TCO_pred), TCO_pred.device
    obj_h = np.asarray(obj_ids.cpu() if isinstance(obj_ids, torch.Tensor) else obj_ids, dtype=np.int64).reshape(-1)
    view_h = np.asarray(view_ids.cpu() if isinstance(view_ids, torch.Tensor) else view_ids, dtype=np.int64).reshape(-1)
    assert TCO_pred.shape == (B, 4, 4) and TCO_gt.shape == (B, 4, 4) and K.dim() == 3 and K.shape[1:] == (3, 3) and len(obj_h) == B and len(view_h) == B
    if B and (obj_h.min() < 0 or obj_h.max() >= len(models.labels)):
        raise ValueError(f'obj_ids outside [0, {len(models.labels)})')
    if B and (view_h.min() < 0 or view_h.max() >= len(K)):
        raise ValueError(f'view_ids outside [0, {len(K)})')
    obj, view = ints_to_device(obj_h.astype(np.int32), dev), ints_to_device(view_h.astype(np.int32), dev)
    mssd, mspd = mssd_mspd(TCO_pred, TCO_gt, obj, view, K, models)
    depth = depth.detach().float().contiguous()
    assert depth.dim() == 3 and depth.shape[0] == len(K), depth.shape
    taus_abs = host_to_device(absolute_taus(taus, obj_h, models.diameters), dev)
    counts = vsd_counts(TCO_pred, TCO_gt, obj, view, K, depth, models, taus_abs, delta, max_workspace_bytes)
    return dict(mssd=mssd, mspd=mspd, vsd_counts=counts, vsd=vsd_from_counts(counts))


class _CallableModule(types.ModuleType):
    """`cosypose_amd.bop_errors` names this module once it is imported and the function before: calling either is the function"""

    def __call__(self, *args, **kwargs):
        return bop_errors(*args, **kwargs)

    __call__.__doc__ = bop_errors.__doc__


__signature__ = inspect.signature(bop_errors)                        # what inspect.signature(cosypose_amd.bop_errors) shows
__doc__ += '\nCalling the module is calling bop_errors:\n\n    bop_errors' + str(__signature__) + '\n\n    ' + bop_errors.__doc__
sys.modules[__name__].__class__ = _CallableModule
