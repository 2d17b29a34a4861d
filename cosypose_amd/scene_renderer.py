"""On-device scene renderer with the interface of the reference's BulletSceneRenderer
(cosypose/rendering/bullet_scene_renderer.py:12-64): `render_scene(obj_infos, cam_infos, render_depth=False)` -> one dict per camera
with `rgb` (H,W,3) uint8, `mask` (H,W) int32 and, when asked, `depth` (H,W) float32.  It is what the reference's figures
(visualization/singleview.py, multiview.py) and the instance masks / `visib_fract` of the BOP datasets are made with.

Many object instances in many views meet in ONE z-buffer per view (csrc/kernels_scene.hip); the per-pixel arithmetic and the shading
are the batch rasteriser's (HipBatchRenderer, bit for bit), so camera model, near plane and non-finite poses behave as there and pixel
VALUES are parity-unpinned as there (PyBullet's OpenGL shading is third-party).

`render` is the device interface (tensors in, tensors out, any number of views of one resolution), `render_scene` the reference's
host interface on top of it, `scene_visibility` the companion of MultiviewScenePredictor.reproject_scene: which object is seen in
which view, and how much of it.

"Visible" here means: the pixel is won by the instance in the rendered scene's z-buffer.  BOP's dataset tool compares with the SENSOR
depth under a 15 mm tolerance instead and counts the part of the silhouette outside the frame: that is cosypose_amd.gt_info /
annotate_gt (gt_annotations.py), which take a measured depth frame -- or, for a scene without a sensor, this renderer's own
render(..., render_depth=True)['depth'].
"""
import ctypes

import numpy as np
import torch

from ._lib import lib, check, ptr, stream, require_device, host_to_device, CosyHipError
from .rasterizer import make_shade


def plan_scene(obj_infos, cam_infos, label_to_id=None):
    """The host half of render_scene, no device needed: one launch group per distinct image size.
    -> list of dicts, in order of first appearance of the size: resolution (H, W), cam_ids (indices into cam_infos), and the rows of
    the launch, view-major / object-minor: obj_index (N,) index into obj_infos, view_ids (N,) index into cam_ids, labels (N,),
    obj_ids (N,) int32 (with label_to_id), TCO (N,4,4) float32 = inv(TWC) TWO formed in float64 and rounded once, K (n_views,3,3)
    float32, colors (N,4) float32 or None (rows without a colour: alpha -1 = the mesh's own colours)."""
    TWO = np.stack([np.asarray(o['TWO'], np.float64).reshape(4, 4) for o in obj_infos]) if len(obj_infos) else np.zeros((0, 4, 4))
    labels = np.array([o['name'] for o in obj_infos], dtype=object)
    n_obj = len(obj_infos)
    colors = None
    if any(o.get('color') is not None for o in obj_infos):
        colors = np.full((n_obj, 4), -1.0, np.float32)
        for i, o in enumerate(obj_infos):
            if o.get('color') is not None:
                c = np.asarray(o['color'], np.float32).reshape(-1)
                colors[i, :3] = c[:3]
                colors[i, 3] = max(float(c[3]), 0.0) if len(c) > 3 else 1.0      # the alpha VALUE is ignored: >= 0 only says "override"
    groups = {}
    for c, cam in enumerate(cam_infos):
        res = tuple(int(r) for r in cam['resolution'])
        groups.setdefault((min(res), max(res)), []).append(c)           # simulator/camera.py:46: the image is (min(res), max(res))
    plans = []
    for (H, W), cam_ids in groups.items():
        TCW = np.stack([np.linalg.inv(np.asarray(cam_infos[c]['TWC'], np.float64).reshape(4, 4)) for c in cam_ids])
        TCO = (TCW[:, None] @ TWO[None]).reshape(-1, 4, 4).astype(np.float32)
        obj_index = np.tile(np.arange(n_obj), len(cam_ids))
        plan = dict(resolution=(H, W), cam_ids=list(cam_ids), obj_index=obj_index, view_ids=np.repeat(np.arange(len(cam_ids)), n_obj).astype(np.int32),
                    labels=labels[obj_index], TCO=TCO, K=np.stack([np.asarray(cam_infos[c]['K'], np.float64).reshape(3, 3) for c in cam_ids]).astype(np.float32),
                    colors=None if colors is None else colors[obj_index])
        if label_to_id is not None:
            plan['obj_ids'] = np.array([label_to_id[l] for l in plan['labels']], np.int32).reshape(-1)
        plans.append(plan)
    return plans


class HipSceneRenderer:
    """meshes: RenderMeshes on the device.  background_color: 8-bit values as the reference's (`im[mask] = background_color` on its
    uint8 image): (0, 0, 0) .. (255, 255, 255); `render` returns them / 255.  shading / ambient / diffuse / light_dir: as
    HipBatchRenderer, from the same table."""

    def __init__(self, meshes, background_color=(0, 0, 0), shading='flat', ambient=None, diffuse=None, light_dir=None):
        self.meshes = meshes
        self.background_color = tuple(float(c) for c in background_color)
        assert len(self.background_color) == 3
        self._background = (ctypes.c_float * 3)(*(np.asarray(self.background_color, np.float32) / np.float32(255.0)))
        self.shade, _ = make_shade(shading, ambient, diffuse, light_dir)
        self._scratch = {}       # per HIP stream: renders issued on different streams may overlap

    def render(self, labels, view_ids, TCO, K, resolution, colors=None, render_depth=False, render_mask=False, stats=False):
        """labels (N,) object names, view_ids (N,) ints in [0, n_views) (host values: they are ranked on the host), TCO (N,4,4) and
        K (n_views,3,3) device tensors, resolution (H, W); colors (N,4) device tensor or None: a row with alpha >= 0 is drawn in its
        rgb instead of the mesh's vertex colours and texture (the alpha value itself is ignored -- nothing is blended), alpha < 0
        keeps the mesh's own.  Rows in any order; a view may have none.
        -> dict: rgb (n_views,3,H,W) float32 in [0,1]; depth (n_views,H,W) metres, 0 = background; mask (n_views,H,W) int32 row
        index of the winner, -1 = background; with stats: px_count_all / px_count_visib (N,) int32, visib_fract (N,) float32 =
        visib / all (0 where all = 0), bbox_obj / bbox_visib (N,4) float32 xyxy inclusive pixel indices, -1 when empty.  Entries not
        asked for are None."""
        m = self.meshes
        require_device(m.verts, TCO, K, colors)
        H, W = int(resolution[0]), int(resolution[1])
        TCO = torch.as_tensor(TCO).detach().float().contiguous()
        K = torch.as_tensor(K).detach().float().contiguous()
        n, n_views = len(TCO), len(K)
        dev = K.device
        obj = np.ascontiguousarray(np.fromiter((m.label_to_id[l] for l in labels), dtype=np.int32, count=n))
        view = np.ascontiguousarray(np.asarray(view_ids.cpu() if isinstance(view_ids, torch.Tensor) else view_ids, dtype=np.int32).reshape(-1))
        assert TCO.shape == (n, 4, 4) and K.shape == (n_views, 3, 3) and len(view) == n, (TCO.shape, K.shape, len(view))
        if colors is not None:
            colors = torch.as_tensor(colors).detach().float().contiguous()
            assert colors.shape == (n, 4), colors.shape
        need = lib().cosy_render_scene_scratch_bytes(n, n_views, m.verts.shape[1], H, W)
        key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
        scratch = self._scratch.get(key)
        if scratch is None or scratch.numel() < need:
            scratch = self._scratch[key] = torch.empty(max(need, 32), dtype=torch.uint8, device=dev)
        out = dict(rgb=torch.empty(n_views, 3, H, W, device=dev), depth=None, mask=None, px_count_all=None, px_count_visib=None, visib_fract=None,
                   bbox_obj=None, bbox_visib=None)
        if render_depth:
            out['depth'] = torch.empty(n_views, H, W, device=dev)
        if render_mask:
            out['mask'] = torch.empty(n_views, H, W, device=dev, dtype=torch.int32)
        if stats:
            out.update(px_count_all=torch.empty(n, device=dev, dtype=torch.int32), px_count_visib=torch.empty(n, device=dev, dtype=torch.int32),
                       bbox_obj=torch.empty(n, 4, device=dev), bbox_visib=torch.empty(n, 4, device=dev))
        mesh = m.c_struct()
        check(lib().cosy_render_scene(ctypes.byref(mesh), ctypes.byref(self.shade), obj.ctypes.data, view.ctypes.data, ptr(TCO), ptr(colors), ptr(K),
                                      n, n_views, H, W, self._background, ptr(out['rgb']), ptr(out['depth']), ptr(out['mask']),
                                      ptr(out['px_count_all']), ptr(out['px_count_visib']), ptr(out['bbox_obj']), ptr(out['bbox_visib']),
                                      ptr(scratch), stream()))
        if stats:
            n_all = out['px_count_all'].float()
            out['visib_fract'] = torch.where(n_all > 0, out['px_count_visib'].float() / n_all.clamp(min=1.0), torch.zeros_like(n_all))
        return out

    def render_scene(self, obj_infos, cam_infos, render_depth=False):
        """BulletSceneRenderer.render_scene: obj_infos = dicts with `name`, `TWO` (4,4) and optionally `color` (rgba, alpha ignored);
        cam_infos = dicts with `K` (3,3), `TWC` (4,4), `resolution`.  -> one dict per camera: rgb (H,W,3) uint8 = floor(255 x + 0.5),
        mask (H,W) int32 = index into obj_infos of the instance seen, -1 = background (PyBullet's mask holds its body ids there), and
        with render_depth depth (H,W) float32 in metres, 0 = background.  One launch per distinct resolution."""
        dev = self.meshes.verts.device
        if dev.type != 'cuda':
            raise CosyHipError('cosypose_amd runs on a ROCm device only (the meshes are on the CPU); there is no CPU fallback')
        obs = [None] * len(cam_infos)
        n_obj = len(obj_infos)
        for plan in plan_scene(obj_infos, cam_infos):
            out = self.render(plan['labels'], plan['view_ids'], host_to_device(plan['TCO'], dev), host_to_device(plan['K'], dev), plan['resolution'],
                              colors=None if plan['colors'] is None else host_to_device(plan['colors'], dev), render_depth=render_depth,
                              render_mask=True)
            rgb = torch.floor(out['rgb'] * 255.0 + 0.5).to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()
            mask = out['mask'].cpu().numpy()
            depth = out['depth'].cpu().numpy() if render_depth else None
            for v, c in enumerate(plan['cam_ids']):
                # rows are view-major / object-minor: row index = v * n_obj + object index
                o = dict(rgb=np.ascontiguousarray(rgb[v]), mask=np.where(mask[v] >= 0, mask[v] - v * n_obj, -1).astype(np.int32))
                if render_depth:
                    o['depth'] = depth[v]
                obs[c] = o
        return obs


def scene_visibility(renderer, objects, cameras, resolution):
    """Every object of a scene in every camera, with what is seen of it: the companion of MultiviewScenePredictor.reproject_scene.
    objects: PandasTensorCollection with TWO (n_obj,4,4) and infos `label` (and `obj_id` when present); cameras: TWC, K and infos
    `view_id`; resolution (H, W) of all views.  -> PandasTensorCollection in reproject_scene's row order (object-major, view-minor):
    infos view_id, label, obj_id, px_count_all, px_count_visib, visib_fract; tensors poses (TCO), bboxes (= bbox_visib) and
    bboxes_obj, xyxy inclusive pixel indices, -1 when empty.  One launch."""
    import pandas as pd
    from .bundle_adjustment import invert_T
    from .tensor_collection import PandasTensorCollection
    n_obj, n_cam = len(objects), len(cameras)
    require_device(objects.TWO, cameras.TWC, cameras.K)
    poses = (invert_T(cameras.TWC)[None, :] @ objects.TWO[:, None]).reshape(n_obj * n_cam, 4, 4)
    labels = np.repeat(objects.infos['label'].values, n_cam)
    view_rows = np.tile(np.arange(n_cam, dtype=np.int32), n_obj)
    out = renderer.render(labels, view_rows, poses, cameras.K, resolution, stats=True)
    obj_ids = objects.infos['obj_id'].values if 'obj_id' in objects.infos else np.arange(n_obj)
    infos = pd.DataFrame(dict(view_id=np.tile(cameras.infos['view_id'].values, n_obj), label=labels, obj_id=np.repeat(obj_ids, n_cam),
                              px_count_all=out['px_count_all'].cpu().numpy(), px_count_visib=out['px_count_visib'].cpu().numpy(),
                              visib_fract=out['visib_fract'].cpu().numpy()))
    return PandasTensorCollection(infos=infos, poses=poses, bboxes=out['bbox_visib'], bboxes_obj=out['bbox_obj'])
