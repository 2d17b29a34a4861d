#!/usr/bin/env python3
"""Timing of the scene renderer (cosypose_amd.scene_renderer.HipSceneRenderer.render, csrc/kernels_scene.hip) on one GPU: the 25-object,
8-view scene of cosypose_amd.synthetic.make_ba_scene (the scene of bench_ba.py), every object in every view = 200 rows, meshes of 6016
faces (make_render_meshes, one per BA mesh type, n_lat=48, n_lon=64), 480x640, rgb + depth + mask + statistics in one call.  Prints one
JSON line.  bench.py (the flagship workload) is a different script and is not affected.

    timeout -k 10 600 python bench_scene.py --warmup 2 --runs 7 --out profiles/scene_bench.json

Reported: milliseconds per call (median of the runs, each a window of --calls calls between two device events, all in this process); the same output through the route the package
offered before -- HipBatchRenderer.render(..., render_depth=True) per (view, object) at 480x640 in chunks, then a depth composite and the
statistics in torch -- and the ratio of the two; whether the two routes agree; and the bytes the call must at least move (z-buffer clear
and read, rgb / depth / mask written) over the measured time as a fraction of the HBM bandwidth.
`gate_ok`: the scene call is not slower than the old route by more than the run-to-run spread.
"""
import argparse
import json
import statistics

HBM_GBPS = 8000.0       # MI355X peak, as bench.py


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seed', type=int, default=7)
    ap.add_argument('--objects', type=int, default=25)
    ap.add_argument('--views', type=int, default=8)
    ap.add_argument('--n-lat', type=int, default=48)
    ap.add_argument('--n-lon', type=int, default=64)
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--chunk', type=int, default=50, help='rows per HipBatchRenderer call of the old route')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--runs', type=int, default=7)
    ap.add_argument('--baseline-runs', type=int, default=3)
    ap.add_argument('--calls', type=int, default=50, help='calls per timed window of the scene renderer')
    ap.add_argument('--baseline-calls', type=int, default=5, help='calls per timed window of the old route')
    ap.add_argument('--out', default=None, help='also write the result to this JSON file')
    args = ap.parse_args()

    import numpy as np
    import torch
    from cosypose_amd import build, synthetic as syn
    from cosypose_amd.rasterizer import HipBatchRenderer, RenderMeshes
    from cosypose_amd.scene_renderer import HipSceneRenderer
    assert torch.cuda.is_available(), 'bench_scene.py needs a ROCm device'
    scene = syn.make_ba_scene(args.seed, args.objects, args.views, 8)
    n_mesh = len(scene['n_sym'])
    labels = np.array([f'obj_{i:06d}' for i in range(1, n_mesh + 1)])
    verts, faces, colors = syn.make_render_meshes(args.seed, n_mesh, n_lat=args.n_lat, n_lon=args.n_lon)
    meshes = RenderMeshes(labels, verts, faces, colors).cuda()
    # the objects in the world frame: each object's first candidate, carried there by its view's camera (the scene keeps candidates)
    view_index = {v: i for i, v in enumerate(scene['cam_view_id'])}
    obj_ids = np.unique(scene['cand_obj_id'])
    first = [int(np.flatnonzero(scene['cand_obj_id'] == o)[0]) for o in obj_ids]
    TWO = np.stack([scene['cam_TWC'][view_index[scene['cand_view_id'][c]]] @ scene['cand_poses'][c] for c in first])
    obj_label = labels[scene['cand_label_id'][first]]
    n_obj, n_views, H, W = len(obj_ids), args.views, args.height, args.width
    TCO = (np.linalg.inv(scene['cam_TWC'])[:, None] @ TWO[None]).reshape(-1, 4, 4).astype(np.float32)      # view-major, object-minor
    row_view = np.repeat(np.arange(n_views), n_obj).astype(np.int32)
    row_label = np.tile(obj_label, n_views)
    N = len(TCO)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    TCO_d, K_d = d(TCO), d(scene['cam_K'].astype(np.float32))
    K_rows = K_d[torch.from_numpy(row_view).long().cuda()].contiguous()
    scene_renderer, batch_renderer = HipSceneRenderer(meshes), HipBatchRenderer(meshes)
    infos = [dict(name=l) for l in row_label]

    def timed(fn, calls):
        """ms per call over a window of `calls` calls between two device events (a single call of well under a millisecond would
        measure the clock as much as the work)"""
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(calls):
            out = fn()
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end) / calls, out

    new = lambda: scene_renderer.render(row_label, row_view, TCO_d, K_d, (H, W), render_depth=True, render_mask=True, stats=True)

    def box(m):
        """xyxy of inclusive pixel indices of a (n,H,W) bool stack, -1 when empty"""
        xs, ys = m.any(1), m.any(2)
        ax, ay = torch.arange(W, device='cuda'), torch.arange(H, device='cuda')
        big = 1 << 30
        b = torch.stack([torch.where(xs, ax, big).amin(1), torch.where(ys, ay, big).amin(1), torch.where(xs, ax, -1).amax(1),
                         torch.where(ys, ay, -1).amax(1)], 1).float()
        return torch.where(xs.any(1)[:, None], b, torch.full_like(b, -1.0))

    def old():
        """one full-frame render per row, then the composite: nearest depth per view, ties to the row that comes first"""
        rgb = torch.empty(n_views, 3, H, W, device='cuda'); depth = torch.empty(n_views, H, W, device='cuda')
        mask = torch.empty(n_views, H, W, device='cuda', dtype=torch.int32)
        n_all = torch.empty(N, device='cuda', dtype=torch.int32); n_vis = torch.empty_like(n_all)
        b_obj = torch.empty(N, 4, device='cuda'); b_vis = torch.empty(N, 4, device='cuda')
        for v in range(n_views):
            rows = np.flatnonzero(row_view == v)
            r_rgb, r_depth = [], []
            for c in range(0, len(rows), args.chunk):
                sel = rows[c:c + args.chunk]
                a, b = batch_renderer.render([infos[i] for i in sel], TCO_d[sel[0]:sel[-1] + 1], K_rows[sel[0]:sel[-1] + 1], resolution=(H, W),
                                             render_depth=True)
                r_rgb.append(a); r_depth.append(b)
            r_rgb, r_depth = torch.cat(r_rgb), torch.cat(r_depth)
            hit = r_depth > 0
            zmin, win = torch.where(hit, r_depth, torch.full_like(r_depth, float('inf'))).min(0)       # first index of the minimum
            fg = torch.isfinite(zmin)
            depth[v] = torch.where(fg, zmin, torch.zeros_like(zmin))
            rgb[v] = torch.gather(r_rgb, 0, win[None, None].expand(1, 3, H, W))[0] * fg
            mask[v] = torch.where(fg, win + int(rows[0]), torch.full_like(win, -1)).int()
            vis = (mask[v][None] == torch.as_tensor(rows, device='cuda', dtype=torch.int32)[:, None, None])
            n_all[rows[0]:rows[-1] + 1] = hit.sum((1, 2)).int(); n_vis[rows[0]:rows[-1] + 1] = vis.sum((1, 2)).int()
            b_obj[rows[0]:rows[-1] + 1] = box(hit); b_vis[rows[0]:rows[-1] + 1] = box(vis)
        fract = torch.where(n_all > 0, n_vis.float() / n_all.float().clamp(min=1.0), torch.zeros(N, device='cuda'))
        return dict(rgb=rgb, depth=depth, mask=mask, px_count_all=n_all, px_count_visib=n_vis, visib_fract=fract, bbox_obj=b_obj, bbox_visib=b_vis)

    for _ in range(args.warmup):
        new()
    runs = [timed(new, args.calls) for _ in range(args.runs)]
    if args.warmup:
        old()
    base = [timed(old, args.baseline_calls) for _ in range(args.baseline_runs)]
    ms, base_ms = statistics.median(r[0] for r in runs), statistics.median(r[0] for r in base)
    spread = max(max(r[0] for r in runs) - min(r[0] for r in runs), max(r[0] for r in base) - min(r[0] for r in base))
    a, b = runs[-1][1], base[-1][1]
    differ = {k: int((a[k] != b[k]).sum()) for k in a}
    min_bytes = n_views * H * W * (8 + 8 + 12 + 4 + 4)          # z-buffer cleared and read, rgb + depth + mask written
    from cosypose_amd._lib import lib
    stamp = build.read_stamp() or {}
    result = {
        'metric': 'scene render, HipSceneRenderer.render (rgb + depth + mask + statistics, one call)', 'value': round(ms, 3), 'unit': 'ms/call',
        'higher_is_better': False, 'runs_ms': [round(r[0], 3) for r in runs],
        'per_row_route_ms': round(base_ms, 3), 'per_row_route_runs_ms': [round(r[0], 3) for r in base], 'speedup_vs_per_row_route': round(base_ms / ms, 3),
        'run_to_run_spread_ms': round(spread, 3), 'gate_ok': bool(ms <= base_ms + spread),
        'values_that_differ_from_per_row_route': differ,
        'min_bytes_moved': min_bytes, 'fraction_of_hbm_bandwidth': round(min_bytes / (ms * 1e-3) / (HBM_GBPS * 1e9), 5), 'hbm_peak_gbps': HBM_GBPS,
        'scratch_bytes': int(lib().cosy_render_scene_scratch_bytes(N, n_views, meshes.verts.shape[1], H, W)),
        'per_row_route_scratch_bytes_per_chunk': int(lib().cosy_render_scratch_bytes(min(args.chunk, n_obj), meshes.verts.shape[1], H, W)),
        'visible_fraction_mean': round(float(a['visib_fract'].mean()), 4), 'foreground_share': round(float((a['mask'] >= 0).float().mean()), 4),
        'config': {'seed': args.seed, 'objects': int(n_obj), 'views': n_views, 'rows': int(N), 'faces_per_mesh': int(meshes.faces.shape[1]),
                   'vertices_per_mesh': int(meshes.verts.shape[1]), 'resolution': [H, W], 'chunk': args.chunk, 'warmup': args.warmup, 'runs': args.runs, 'calls_per_run': args.calls, 'baseline_calls_per_run': args.baseline_calls,
                   'baseline_runs': args.baseline_runs},
        'device': torch.cuda.get_device_name(0), 'src_sha': stamp.get('src_sha'),
    }
    line = json.dumps(result)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(result, indent=1) + '\n')
    print(line)


if __name__ == '__main__':
    main()
