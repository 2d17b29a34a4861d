"""BOP ground-truth annotations on the device: per instance the pixel counts, visib_fract, bbox_obj / bbox_visib and the visible masks that
the BOP toolkit's calc_gt_masks.py and calc_gt_info.py write into scene_gt_info.json, mask/ and mask_visib/ -- what BOPDataset
(cosypose/datasets/bop.py:124-153) asks of a scene and what BopScoreMeter / DetectionMeter filter their ground truth by.  HIP:
csrc/kernels_gt.hip behind cosy_gt_info, on the depth windows of csrc/kernels_bop.hip; DESIGN.md section 19 holds the contract,
tests/gt_ref.py its numpy twin.

The toolkit is not part of the reference checkout: the contract is its published definition (visibility mode bop19), restated -- the
depth images are the package's own renders, not the toolkit's.  Every instance is drawn alone on a canvas of 3H x 3W whose centre third
is the frame, so px_count_all and bbox_obj include the part of the silhouette outside the frame; visible means in front of the
measured depth within `delta`, or where the measured depth is missing.  A scene without a sensor passes
HipSceneRenderer.render(..., render_depth=True)['depth'] as the measured depth.
"""
import numpy as np
import torch

from ._lib import lib, check, ptr, stream, require_device, ints_to_device, host_to_device
from .bop_errors import VSD_DELTA, instance_boxes, render_windows

MAX_IDS = 255                        # id_in_segm lives in a uint8 mask, 0 = background


def id_in_segm_of(view_ids):
    """(N,) int32: 1 + the rank of every row among the rows of its view, in row order (the `n + 1` of cosypose/datasets/bop.py:151-153).
    More than 255 rows of one view are refused."""
    view_ids = np.asarray(view_ids, dtype=np.int64).reshape(-1)
    out = np.zeros(len(view_ids), dtype=np.int32)
    seen = {}
    for n, v in enumerate(view_ids.tolist()):
        seen[v] = out[n] = seen.get(v, 0) + 1
    if len(out) and out.max() > MAX_IDS:
        worst = max(seen, key=seen.get)
        raise ValueError(f'view {worst} holds {seen[worst]} instances; the uint8 instance mask holds ids 1..{MAX_IDS}')
    return out


def plan_chunks(boxes, max_pixels=None):
    """The host half of the canvas windows, no device needed.  boxes (N,4) int x0, y0, x1, y1 inclusive on the canvas (empty: x1 < x0 or
    y1 < y0), max_pixels the cap of the window store or None.
    -> list of chunks dict(lo, hi, win_offset (hi - lo,) int64, n_pixels): instances [lo, hi) are worked off while exactly their windows
    are in the store (win_offset = -1: no window).  Every instance is in exactly one chunk; one whose window alone exceeds the cap is
    refused."""
    boxes = np.asarray(boxes, dtype=np.int64).reshape(-1, 4)
    size = np.maximum(boxes[:, 2] - boxes[:, 0] + 1, 0) * np.maximum(boxes[:, 3] - boxes[:, 1] + 1, 0)
    N = len(boxes)

    def chunk(lo, hi):
        s = size[lo:hi]
        return dict(lo=lo, hi=hi, win_offset=np.where(s > 0, np.cumsum(s) - s, -1).astype(np.int64), n_pixels=int(s.sum()))

    if N == 0:
        return []
    if max_pixels is None or int(size.sum()) <= max_pixels:
        return [chunk(0, N)]
    chunks, lo, total = [], 0, 0
    for n in range(N):
        if int(size[n]) > max_pixels:
            raise ValueError(f'max_workspace_bytes holds {max_pixels} window pixels; instance {n} alone needs {int(size[n])} '
                             f'({4 * int(size[n])} bytes)')
        if total + int(size[n]) > max_pixels:
            chunks.append(chunk(lo, n))
            lo, total = n, 0
        total += int(size[n])
    chunks.append(chunk(lo, N))
    return chunks


def canvas_K(K, resolution):
    """K' of the 3H x 3W canvas whose centre third is the frame: cx + W, cy + H, one float32 addition each"""
    H, W = resolution
    Kc = K.clone()
    Kc[:, 0, 2] += float(W)
    Kc[:, 1, 2] += float(H)
    return Kc


def xywh_to_xyxy(boxes):
    """[x, y, w, h] -> [x, y, x + w, y + h] float32 (cosypose/datasets/bop.py:136-144)"""
    b = boxes.to(torch.float32)
    return torch.stack([b[..., 0], b[..., 1], b[..., 0] + b[..., 2], b[..., 1] + b[..., 3]], -1)


def _host_ids(ids):
    return np.asarray(ids.cpu() if isinstance(ids, torch.Tensor) else ids, dtype=np.int64).reshape(-1)


def gt_info(TCO, obj_ids, view_ids, K, depth, models, delta=VSD_DELTA, dense_masks=False, max_workspace_bytes=None):
    """N instances: TCO (N,4,4) device tensor, obj_ids (N,) rows of `models` (BopModels on the device), view_ids (N,) rows of K
    (n_views,3,3) and of depth (n_views,H,W) float32 metres, 0 = missing; the ids are host values (a device tensor is read back: they are
    checked and ranked here).  delta: the visibility tolerance in metres; max_workspace_bytes caps the store of the canvas windows (the
    instances are then worked off in chunks); dense_masks: also the per-instance masks, 2 N H W bytes.  Ids outside their tables and more
    than 255 instances of one view are refused here.  The host waits for the device once, for the boxes that size the store.
    -> dict of device tensors: px_count_all, px_count_valid, px_count_visib (N,) int32; visib_fract (N,) float64 = px_count_visib /
    px_count_all, 0 where nothing is drawn; bbox_obj, bbox_visib (N,4) int32 x, y, w, h with w = x_max - x_min, both -1 where nothing is
    visible (bbox_obj is the box on the canvas in the frame's coordinates: x, y may be negative); id_in_segm (N,) int32; mask_visib_all
    (n_views,H,W) uint8 = id_in_segm of the instance seen, the highest where several are, 0 = background; with dense_masks mask and
    mask_visib (N,H,W) bool.  An instance with a non-finite entry in its pose or its view's K has zero counts and -1 boxes."""
    m = models.meshes
    require_device(m.verts, TCO, K, depth)
    TCO, K = (torch.as_tensor(t).detach().float().contiguous() for t in (TCO, K))
    depth = depth.detach().float().contiguous()
    N, dev = len(TCO), TCO.device
    obj_h, view_h = _host_ids(obj_ids), _host_ids(view_ids)
    assert TCO.shape == (N, 4, 4) and K.dim() == 3 and K.shape[1:] == (3, 3) and len(obj_h) == N and len(view_h) == N
    assert depth.dim() == 3 and depth.shape[0] == len(K), depth.shape
    if N and (obj_h.min() < 0 or obj_h.max() >= len(models.labels)):
        raise ValueError(f'obj_ids outside [0, {len(models.labels)})')
    if N and (view_h.min() < 0 or view_h.max() >= len(K)):
        raise ValueError(f'view_ids outside [0, {len(K)})')
    ids_h = id_in_segm_of(view_h)
    n_views, H, W = depth.shape
    counts = torch.zeros(N, 3, dtype=torch.int32, device=dev)
    bbox = torch.full((2, N, 4), -1, dtype=torch.int32, device=dev)
    composite = torch.zeros(n_views, H, W, dtype=torch.int32, device=dev)
    masks = torch.zeros(2, N, H, W, dtype=torch.uint8, device=dev) if dense_masks else None
    ids = ints_to_device(ids_h, dev)
    if N:
        obj, view = ints_to_device(obj_h.astype(np.int32), dev), ints_to_device(view_h.astype(np.int32), dev)
        Kc, canvas = canvas_K(K, (H, W)), (3 * H, 3 * W)
        boxes = instance_boxes(TCO, obj, view, Kc, models, canvas)
        cap = None if max_workspace_bytes is None else int(max_workspace_bytes) // 4
        chunks = plan_chunks(boxes.cpu().numpy(), cap)                                 # the one wait
        ws_bytes = lib().cosy_gt_info_workspace_bytes(max(c['hi'] - c['lo'] for c in chunks))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        store = None
        for c in chunks:
            lo, hi = c['lo'], c['hi']
            off = host_to_device(c['win_offset'], dev)
            store = render_windows(TCO[lo:hi], obj[lo:hi], view[lo:hi], Kc, models, canvas, boxes[lo:hi], off, c['n_pixels'], store)
            check(lib().cosy_gt_info(ptr(view[lo:hi]), ptr(ids[lo:hi]), ptr(boxes[lo:hi]), ptr(off), ptr(store), c['n_pixels'], ptr(depth), ptr(K),
                                     float(delta), hi - lo, n_views, H, W, ptr(counts[lo:hi]), ptr(bbox[0, lo:hi]), ptr(bbox[1, lo:hi]),
                                     ptr(composite), ptr(masks[0, lo:hi]) if dense_masks else None,
                                     ptr(masks[1, lo:hi]) if dense_masks else None, ptr(ws), ws_bytes, stream()))
    mask_all = torch.empty(n_views, H, W, dtype=torch.uint8, device=dev)
    check(lib().cosy_gt_composite_u8(ptr(composite), composite.numel(), ptr(mask_all), stream()))
    n_all, n_vis = counts[:, 0].to(torch.float64), counts[:, 2].to(torch.float64)
    out = dict(px_count_all=counts[:, 0].contiguous(), px_count_valid=counts[:, 1].contiguous(), px_count_visib=counts[:, 2].contiguous(),
               visib_fract=torch.where(n_all > 0, n_vis / n_all.clamp(min=1.0), torch.zeros_like(n_all)),
               bbox_obj=bbox[0], bbox_visib=bbox[1], id_in_segm=ids, mask_visib_all=mask_all)
    if dense_masks:
        out['mask'], out['mask_visib'] = masks[0].view(torch.bool), masks[1].view(torch.bool)
    return out


INFO_COLUMNS = ('visib_fract', 'px_count_all', 'px_count_valid', 'px_count_visib', 'id_in_segm')


def annotate_gt(gt_data, cameras, depth, models, delta=VSD_DELTA, max_workspace_bytes=None):
    """gt_data: collection with `poses` (TCO) and infos scene_id, view_id, label; cameras: collection with `K` and infos scene_id,
    view_id, one row per view; depth (len(cameras),H,W) measured depth in metres, 0 = missing, rows as cameras -- as BopScoreMeter.add
    takes them.
    -> (annotated, mask_visib_all): the collection with the infos columns visib_fract, px_count_all, px_count_valid, px_count_visib,
    id_in_segm added and the tensors bbox_obj, bbox_visib (n,4) int32 x, y, w, h and bboxes (n,4) float32 = [x, y, x + w, y + h] of
    bbox_visib beside `poses`: what BopScoreMeter.add and DetectionMeter.add take as ground truth; mask_visib_all (len(cameras),H,W)
    uint8, rows as cameras, holding id_in_segm."""
    from .tensor_collection import PandasTensorCollection
    infos = gt_data.infos
    cam_row = {tuple(k): n for n, k in enumerate(cameras.infos[['scene_id', 'view_id']].itertuples(index=False, name=None))}
    try:
        view_ids = np.array([cam_row[tuple(k)] for k in infos[['scene_id', 'view_id']].itertuples(index=False, name=None)], dtype=np.int32)
    except KeyError as e:
        raise ValueError(f'no camera for (scene_id, view_id) = {e.args[0]}') from None
    try:
        obj_ids = np.array([models.label_to_id[l] for l in infos['label'].values], dtype=np.int32)
    except KeyError as e:
        raise ValueError(f'label {e.args[0]!r} is not in the models') from None
    dev = models.meshes.verts.device
    out = gt_info(gt_data.poses.float().to(dev), obj_ids, view_ids, cameras.K.to(dev), depth.to(dev), models, delta=delta,
                  max_workspace_bytes=max_workspace_bytes)
    infos = infos.copy()
    host = torch.stack([out[k].to(torch.float64) for k in INFO_COLUMNS], 1).cpu().numpy()      # one device -> host copy
    for n, k in enumerate(INFO_COLUMNS):
        infos[k] = host[:, n] if k == 'visib_fract' else host[:, n].astype(np.int64)
    tensors = dict(gt_data.tensors)
    tensors.update(bbox_obj=out['bbox_obj'], bbox_visib=out['bbox_visib'], bboxes=xywh_to_xyxy(out['bbox_visib']))
    return PandasTensorCollection(infos, **tensors), out['mask_visib_all']
