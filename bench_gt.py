#!/usr/bin/env python3
"""Timing of the BOP ground-truth annotations (cosypose_amd.gt_info, csrc/kernels_gt.hip) on one GPU: the 25-object, 8-view scene of
cosypose_amd.synthetic.make_ba_scene (the scene of bench_scene.py), every object in every view = 200 instances, meshes of 6016 faces,
480 x 640; the measured depth is the scene's own render in front of a wall, with an occluding wall over a band of the frame.  Prints one
JSON line.  bench.py (the flagship workload) is a different script and is not affected.

    timeout -k 10 600 python bench_gt.py --warmup 1 --runs 5 --out profiles/gt_bench.json

Reported: milliseconds per gt_info call (median of the runs, device events, all in this process; the host ids, their checks and the one
wait for the boxes inside the timed region) and the same annotations through what the package offered before:
HipBatchRenderer.render(render_depth=True) of every instance on the full 1440 x 1920 canvas in chunks, plus torch operations for the
distance images, masks, counts, boxes and the composite.  `gate_ok`: the fused call is not slower than the composed route by more than
the run-to-run spread.  No speed-up is promised; the agreement of the two routes is reported beside it.
"""
import argparse
import json
import statistics


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seed', type=int, default=7)
    ap.add_argument('--objects', type=int, default=25)
    ap.add_argument('--views', type=int, default=8)
    ap.add_argument('--n-lat', type=int, default=48)
    ap.add_argument('--n-lon', type=int, default=64)
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--dense-masks', action='store_true', help='also the per-instance masks (2 N H W bytes)')
    ap.add_argument('--workspace-mib', type=int, default=1024, help='cap of the canvas-window store')
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--baseline-runs', type=int, default=3)
    ap.add_argument('--baseline-chunk', type=int, default=8, help='instances per full-canvas render of the composed route')
    ap.add_argument('--out', default=None, help='also write the result to this JSON file')
    args = ap.parse_args()

    import numpy as np
    import torch
    from cosypose_amd import build, synthetic as syn, BopModels, HipBatchRenderer, HipSceneRenderer, gt_info
    from cosypose_amd.bop_errors import VSD_DELTA
    from cosypose_amd.gt_annotations import canvas_K
    assert torch.cuda.is_available(), 'bench_gt.py needs a ROCm device'
    scene = syn.make_ba_scene(args.seed, args.objects, args.views, 8)
    n_mesh = len(scene['n_sym'])
    labels = [f'obj_{i:06d}' for i in range(1, n_mesh + 1)]
    verts, faces, colors = syn.make_render_meshes(args.seed, n_mesh, n_lat=args.n_lat, n_lon=args.n_lon)
    models = BopModels(labels, verts, faces, colors_list=colors).cuda()
    # the objects in the world frame: each object's first candidate, carried there by its view's camera (as bench_scene.py)
    view_index = {v: i for i, v in enumerate(scene['cam_view_id'])}
    obj_ids = np.unique(scene['cand_obj_id'])
    first = [int(np.flatnonzero(scene['cand_obj_id'] == o)[0]) for o in obj_ids]
    TWO = np.stack([scene['cam_TWC'][view_index[scene['cand_view_id'][c]]] @ scene['cand_poses'][c] for c in first])
    obj_row = scene['cand_label_id'][first].astype(np.int32)
    n_obj, n_views, H, W = len(obj_ids), args.views, args.height, args.width
    TCO = (np.linalg.inv(scene['cam_TWC'])[:, None] @ TWO[None]).reshape(-1, 4, 4).astype(np.float32)      # view-major, object-minor
    view = np.repeat(np.arange(n_views), n_obj).astype(np.int32)
    obj = np.tile(obj_row, n_views)
    N = len(TCO)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    TCO_d, K_d, view_d = d(TCO), d(scene['cam_K'].astype(np.float32)), d(view).long()
    rendered = HipSceneRenderer(models.meshes).render(np.asarray(labels)[obj], view, TCO_d, K_d, (H, W), render_depth=True)['depth']
    depth = torch.where(rendered > 0, rendered, torch.full_like(rendered, 2.5))      # the scene in front of a wall ...
    depth[:, :, int(0.4 * W):int(0.55 * W)] = 0.25                                   # ... and an occluding wall over a band of the frame
    depth = depth.contiguous()
    cap = args.workspace_mib << 20
    delta = float(np.float32(VSD_DELTA))

    def event():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def fused():
        torch.cuda.synchronize()
        e0 = event()
        out = gt_info(TCO_d, obj, view, K_d, depth, models, delta=VSD_DELTA, dense_masks=args.dense_masks, max_workspace_bytes=cap)
        e1 = event()
        torch.cuda.synchronize()
        return dict(ms=e0.elapsed_time(e1), out=out)

    renderer = HipBatchRenderer(models.meshes)
    infos = [dict(name=labels[o]) for o in obj]
    Kc_d = canvas_K(K_d, (H, W))
    xs = torch.arange(W, device='cuda', dtype=torch.float32)[None, None, :]
    ys = torch.arange(H, device='cuda', dtype=torch.float32)[None, :, None]
    ids = np.zeros(N, np.int32)
    for v in range(n_views):
        ids[view == v] = np.arange(1, (view == v).sum() + 1)
    ids_d = d(ids)

    def dist_image(z, Kb):
        X = (xs - Kb[:, 0, 2, None, None]) * z / Kb[:, 0, 0, None, None]
        Y = (ys - Kb[:, 1, 2, None, None]) * z / Kb[:, 1, 1, None, None]
        return torch.sqrt((X * X + Y * Y) + z * z)

    def xywh(m, x_off, y_off):
        """x, y, w, h (w = max - min) of a (n,h,w) bool stack; the caller blanks the rows without a visible pixel"""
        h, w = m.shape[1:]
        cols, rows = m.any(1), m.any(2)
        ax, ay = torch.arange(w, device='cuda'), torch.arange(h, device='cuda')
        big = 1 << 30
        x0, y0 = torch.where(cols, ax, big).amin(1), torch.where(rows, ay, big).amin(1)
        x1, y1 = torch.where(cols, ax, -1).amax(1), torch.where(rows, ay, -1).amax(1)
        return torch.stack([x0 - x_off, y0 - y_off, x1 - x0, y1 - y0], 1).int()

    def composed():
        """full-canvas renders + torch operations, in chunks of instances"""
        torch.cuda.synchronize()
        e0 = event()
        counts = torch.empty(N, 3, dtype=torch.int32, device='cuda')
        b_obj, b_vis = torch.empty(N, 4, dtype=torch.int32, device='cuda'), torch.empty(N, 4, dtype=torch.int32, device='cuda')
        comp = torch.zeros(n_views, H, W, dtype=torch.int32, device='cuda')
        for lo in range(0, N, args.baseline_chunk):
            hi = min(N, lo + args.baseline_chunk)
            rows = view_d[lo:hi]
            D = renderer.render(infos[lo:hi], TCO_d[lo:hi], Kc_d[rows], (3 * H, 3 * W), render_depth=True)[1]
            drawn = D > 0
            Kb = K_d[rows]
            dg, dt = dist_image(D[:, H:2 * H, W:2 * W], Kb), dist_image(depth[rows], Kb)
            m = dg > 0
            vis = m & (((dg - dt) <= delta) | (dt == 0))
            counts[lo:hi, 0] = drawn.sum((1, 2)); counts[lo:hi, 1] = (m & (dt > 0)).sum((1, 2)); counts[lo:hi, 2] = vis.sum((1, 2))
            seen = (counts[lo:hi, 2] > 0)[:, None]
            b_obj[lo:hi] = torch.where(seen, xywh(drawn, W, H), torch.full_like(b_obj[lo:hi], -1))
            b_vis[lo:hi] = torch.where(seen, xywh(vis, 0, 0), torch.full_like(b_vis[lo:hi], -1))
            painted = vis * ids_d[lo:hi, None, None]
            for v in np.unique(view[lo:hi]):
                comp[v] = torch.maximum(comp[v], painted[torch.from_numpy(view[lo:hi] == v).cuda()].amax(0))
        e1 = event()
        torch.cuda.synchronize()
        return dict(ms=e0.elapsed_time(e1), out=dict(counts=counts, bbox_obj=b_obj, bbox_visib=b_vis, mask_visib_all=comp.to(torch.uint8)))

    for _ in range(args.warmup):
        fused()
    runs = [fused() for _ in range(args.runs)]
    if args.warmup:
        composed()
    base = [composed() for _ in range(args.baseline_runs)]
    med = lambda rows, k: statistics.median(r[k] for r in rows)
    ms, base_ms = med(runs, 'ms'), med(base, 'ms')
    spread = max(max(r['ms'] for r in runs) - min(r['ms'] for r in runs), max(r['ms'] for r in base) - min(r['ms'] for r in base))
    a, b = runs[-1]['out'], base[-1]['out']
    a_counts = torch.stack([a['px_count_all'], a['px_count_valid'], a['px_count_visib']], 1)
    window_px = int(a['px_count_all'].sum())
    stamp = build.read_stamp() or {}
    result = {
        'metric': 'BOP ground-truth annotations, gt_info (counts, boxes, composite mask, one call)', 'value': round(ms, 3), 'unit': 'ms/call',
        'higher_is_better': False, 'runs_ms': [round(r['ms'], 3) for r in runs],
        'composed_route_ms': round(base_ms, 3), 'composed_route_runs_ms': [round(r['ms'], 3) for r in base],
        'speedup_vs_composed_route': round(base_ms / ms, 3), 'run_to_run_spread_ms': round(spread, 3), 'gate_ok': bool(ms <= base_ms + spread),
        'counts_equal_composed_route': bool(torch.equal(a_counts, b['counts'])),
        'boxes_equal_composed_route': bool(torch.equal(a['bbox_obj'], b['bbox_obj']) and torch.equal(a['bbox_visib'], b['bbox_visib'])),
        'composite_equal_composed_route': bool(torch.equal(a['mask_visib_all'], b['mask_visib_all'])),
        'drawn_pixels': window_px, 'visible_fraction_mean': round(float(a['visib_fract'].mean()), 4),
        'instances_without_a_visible_pixel': int((a['px_count_visib'] == 0).sum()),
        'config': {'seed': args.seed, 'objects': int(n_obj), 'views': n_views, 'instances': int(N), 'faces_per_mesh': int(models.meshes.faces.shape[1]),
                   'resolution': [H, W], 'dense_masks': args.dense_masks, 'workspace_mib': args.workspace_mib, 'warmup': args.warmup,
                   'runs': args.runs, 'baseline_runs': args.baseline_runs, 'baseline_chunk': args.baseline_chunk},
        'device': torch.cuda.get_device_name(0), 'src_sha': stamp.get('src_sha'),
    }
    line = json.dumps(result)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(result, indent=1) + '\n')
    print(line)


if __name__ == '__main__':
    main()
