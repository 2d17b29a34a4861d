#!/usr/bin/env python3
"""Timing of the BOP pose errors (cosypose_amd.bop_errors, csrc/kernels_bop.hip) on one GPU, on an evaluation-sized workload: 4096
tentative (estimate, ground truth) pairs -- four estimates per ground truth -- of 21 objects whose meshes hold 2 000 - 40 000 vertices
and 1 - 64 symmetries (both log-uniform), in 8 views of 480 x 640 with a measured depth frame each.  Prints one JSON line.  bench.py
(the flagship workload) is a different script and is not affected.

    timeout -k 10 900 python bench_bop.py --warmup 1 --runs 5 --out profiles/bop_bench.json

Reported: milliseconds per bop_errors call (median of the runs, device events, all in this process) with its split over the three
steps (MSSD + MSPD; boxes, the host read and the depth windows; the VSD counts) from a second, instrumented pass, and the same pairs through what the package offered
before: HipBatchRenderer.render(render_depth=True) of every estimate and ground truth at full frame plus torch operations for the
distance images, masks and counts, and broadcast torch operations for MSSD / MSPD.  `gate_ok`: the fused call is not slower than the
composed route by more than the run-to-run spread.  No speed-up is promised; the agreement of the two routes is reported beside it.
"""
import argparse
import json
import statistics


def sphere_mesh(seed, n_verts):
    """a bumpy ellipsoid of about n_verts vertices (synthetic.make_render_meshes with the grid sized to it)"""
    from cosypose_amd import synthetic as syn
    n_lon = max(8, int(round((2.0 * n_verts) ** 0.5)))
    n_lat = max(4, int(round((n_verts - 2) / n_lon)) + 1)
    v, f, c = syn.make_render_meshes(seed, 1, n_lat, n_lon)
    return v[0], f[0], c[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seed', type=int, default=3)
    ap.add_argument('--pairs', type=int, default=4096)
    ap.add_argument('--objects', type=int, default=21)
    ap.add_argument('--views', type=int, default=8)
    ap.add_argument('--min-verts', type=int, default=2000)
    ap.add_argument('--max-verts', type=int, default=40000)
    ap.add_argument('--max-sym', type=int, default=64)
    ap.add_argument('--height', type=int, default=480)
    ap.add_argument('--width', type=int, default=640)
    ap.add_argument('--workspace-mib', type=int, default=1024, help='cap of the depth-window store')
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--baseline-runs', type=int, default=3)
    ap.add_argument('--baseline-chunk', type=int, default=128, help='pairs per full-frame render of the composed route')
    ap.add_argument('--out', default=None, help='also write the result to this JSON file')
    args = ap.parse_args()

    import numpy as np
    import torch
    from cosypose_amd import build, synthetic as syn, BopModels, HipBatchRenderer, HipSceneRenderer
    from cosypose_amd import bop_errors as be
    assert torch.cuda.is_available(), 'bench_bop.py needs a ROCm device'
    rs = np.random.RandomState(args.seed)
    H, W, B = args.height, args.width, args.pairs
    n_verts = np.exp(rs.uniform(np.log(args.min_verts), np.log(args.max_verts), args.objects)).astype(int)
    n_verts[0], n_verts[-1] = args.min_verts, args.max_verts
    n_sym = np.exp(rs.uniform(0, np.log(args.max_sym), args.objects)).astype(int)
    n_sym[0], n_sym[-1] = 1, args.max_sym
    meshes = [sphere_mesh(args.seed + o, int(n)) for o, n in enumerate(n_verts)]
    syms = []
    for S in n_sym:
        s = np.tile(np.eye(4), (S, 1, 1))
        for k in range(1, S):
            a = 2 * np.pi * k / S
            s[k, :2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
        syms.append(s)
    labels = [f'obj_{o + 1:06d}' for o in range(args.objects)]
    models = BopModels(labels, [m[0] for m in meshes], [m[1] for m in meshes], symmetries=syms, colors_list=[m[2] for m in meshes]).cuda()
    n_gt = max(1, B // 4)
    gt_of_pair = np.arange(B) // 4
    obj_gt, view_gt = rs.randint(0, args.objects, n_gt), rs.randint(0, args.views, n_gt)
    T_gt = syn.make_TCO(args.seed + 1, n_gt)
    noise = np.stack([syn._rigid_noise(rs, 0.05, 0.01) for _ in range(B)])
    Tg = T_gt[gt_of_pair]
    Tp = (Tg.astype(np.float64) @ noise).astype(np.float32)
    obj, view = obj_gt[gt_of_pair].astype(np.int32), view_gt[gt_of_pair].astype(np.int32)
    K = syn.make_K(args.views, H, W)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    Tp_d, Tg_d, obj_d, view_d, K_d = d(Tp), d(Tg), d(obj), d(view), d(K)
    scene = HipSceneRenderer(models.meshes).render(np.asarray(labels)[obj_gt], view_gt, d(T_gt), K_d, (H, W), render_depth=True)['depth']
    depth = torch.where(scene > 0, scene, torch.full_like(scene, 2.5)).contiguous()          # the ground-truth scene in front of a wall
    taus_abs = d(be.absolute_taus(be.VSD_TAUS, obj, models.diameters))
    cap = args.workspace_mib << 20

    def event():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def fused():
        """the public call as a user makes it: host ids in, the id checks, the taus and their upload inside the timed region"""
        torch.cuda.synchronize()
        e0 = event()
        out = be.bop_errors(Tp_d, Tg_d, obj, view, K_d, depth, models, taus=be.VSD_TAUS, delta=be.VSD_DELTA, max_workspace_bytes=cap)
        e1 = event()
        torch.cuda.synchronize()
        return dict(ms=e0.elapsed_time(e1), out=out)

    def split():
        """a second, instrumented pass over the call's two halves (events between the steps): where the time goes"""
        torch.cuda.synchronize()
        e0 = event()
        be.mssd_mspd(Tp_d, Tg_d, obj_d, view_d, K_d, models)
        marks = []
        be.vsd_counts(Tp_d, Tg_d, obj_d, view_d, K_d, depth, models, taus_abs, be.VSD_DELTA, cap, timings=marks)
        e1 = event()
        torch.cuda.synchronize()
        windows = sum(marks[i].elapsed_time(marks[i + 1]) for i in range(0, len(marks) - 1, 2))
        pairs = sum(marks[i].elapsed_time(marks[i + 1]) for i in range(1, len(marks) - 1, 2))
        return dict(ms=e0.elapsed_time(e1), mssd_mspd_ms=e0.elapsed_time(marks[0]), windows_ms=windows, vsd_ms=pairs, chunks=(len(marks) - 1) // 2)

    renderer = HipBatchRenderer(models.meshes)
    infos = [dict(name=labels[o]) for o in obj]
    xs = torch.arange(W, device='cuda', dtype=torch.float32)[None, None, :]
    ys = torch.arange(H, device='cuda', dtype=torch.float32)[None, :, None]

    def dist_image(z, Kb):
        X = (xs - Kb[:, 0, 2, None, None]) * z / Kb[:, 0, 0, None, None]
        Y = (ys - Kb[:, 1, 2, None, None]) * z / Kb[:, 1, 1, None, None]
        return torch.sqrt((X * X + Y * Y) + z * z)

    def composed():
        """full-frame renders + torch operations, in chunks of pairs; MSSD / MSPD by broadcast torch operations per object"""
        torch.cuda.synchronize()
        e0 = event()
        counts = torch.empty(B, 2 + taus_abs.shape[1], dtype=torch.int32, device='cuda')
        for lo in range(0, B, args.baseline_chunk):
            hi = min(B, lo + args.baseline_chunk)
            Kb = K_d[view_d[lo:hi].long()]
            de = dist_image(renderer.render(infos[lo:hi], Tp_d[lo:hi], Kb, (H, W), render_depth=True)[1], Kb)
            dg = dist_image(renderer.render(infos[lo:hi], Tg_d[lo:hi], Kb, (H, W), render_depth=True)[1], Kb)
            dt = dist_image(depth[view_d[lo:hi].long()], Kb)
            vis = lambda m: (m > 0) & (((m - dt) <= be.VSD_DELTA) | (dt == 0))
            v_gt = vis(dg)
            v_est = vis(de) | (v_gt & (de > 0))
            inter, diff = v_gt & v_est, (dg - de).abs()
            counts[lo:hi, 0] = (v_gt | v_est).sum((1, 2))
            counts[lo:hi, 1] = inter.sum((1, 2))
            for k in range(taus_abs.shape[1]):
                counts[lo:hi, 2 + k] = (inter & (diff >= taus_abs[lo:hi, k, None, None])).sum((1, 2))
        mssd, mspd = torch.empty(B, device='cuda'), torch.empty(B, device='cuda')
        for o in range(args.objects):
            ids = np.flatnonzero(obj == o)
            V, S = int(models.n_verts[o]), int(models.n_sym[o])
            x = models.meshes.verts[o, :V]
            sym = models.sym_table[o, :S]
            step = max(1, (1 << 24) // (V * S))
            for a in range(0, len(ids), step):
                sel = torch.from_numpy(ids[a:a + step]).cuda()
                P, G, Kb = Tp_d[sel], Tg_d[sel][:, None] @ sym[None], K_d[view_d[sel].long()]                         # G (b,S,4,4)
                q = (x @ P[:, :3, :3].transpose(1, 2) + P[:, None, :3, 3])[:, None]                                 # (b,1,V,3)
                g = x @ G[:, :, :3, :3].transpose(2, 3) + G[:, :, None, :3, 3]                                       # (b,S,V,3)
                f, c = torch.stack([Kb[:, 0, 0], Kb[:, 1, 1]], -1)[:, None, None], Kb[:, None, None, :2, 2]
                mssd[sel] = (q - g).norm(dim=-1).amax(-1).amin(-1)
                mspd[sel] = ((f * q[..., :2] / q[..., 2:] + c) - (f * g[..., :2] / g[..., 2:] + c)).norm(dim=-1).amax(-1).amin(-1)
        e1 = event()
        torch.cuda.synchronize()
        return dict(ms=e0.elapsed_time(e1), out=dict(mssd=mssd, mspd=mspd, vsd_counts=counts))

    for _ in range(args.warmup):
        fused()
    runs = [fused() for _ in range(args.runs)]
    parts = [split() for _ in range(args.baseline_runs)]
    if args.warmup:
        composed()
    base = [composed() for _ in range(args.baseline_runs)]
    med = lambda rows, k: statistics.median(r[k] for r in rows)
    ms, base_ms = med(runs, 'ms'), med(base, 'ms')
    spread = max(max(r['ms'] for r in runs) - min(r['ms'] for r in runs), max(r['ms'] for r in base) - min(r['ms'] for r in base))
    a, b = runs[-1]['out'], base[-1]['out']
    stamp = build.read_stamp() or {}
    result = {
        'metric': 'BOP pose errors, bop_errors (MSSD, MSPD, VSD counts, one call)', 'value': round(ms, 3), 'unit': 'ms/call', 'higher_is_better': False,
        'runs_ms': [round(r['ms'], 3) for r in runs],
        'split_ms': {k: round(med(parts, k), 3) for k in ('mssd_mspd_ms', 'windows_ms', 'vsd_ms')}, 'split_pass_ms': round(med(parts, 'ms'), 3),
        'window_chunks': parts[-1]['chunks'],
        'composed_route_ms': round(base_ms, 3), 'composed_route_runs_ms': [round(r['ms'], 3) for r in base],
        'speedup_vs_composed_route': round(base_ms / ms, 3), 'run_to_run_spread_ms': round(spread, 3), 'gate_ok': bool(ms <= base_ms + spread),
        'vsd_counts_equal_composed_route': bool(torch.equal(a['vsd_counts'], b['vsd_counts'])),
        'max_rel_diff_mssd_vs_composed_route': float(((a['mssd'] - b['mssd']).abs() / b['mssd'].clamp(min=1e-12)).max()),
        'max_abs_diff_mspd_px_vs_composed_route': float((a['mspd'] - b['mspd']).abs().max()),
        'mean_union_pixels': float(a['vsd_counts'][:, 0].float().mean()),
        'config': {'seed': args.seed, 'pairs': B, 'objects': args.objects, 'views': args.views, 'resolution': [H, W],
                   'n_verts': [int(n) for n in models.n_verts.cpu()], 'n_sym': [int(n) for n in n_sym], 'workspace_mib': args.workspace_mib,
                   'warmup': args.warmup, 'runs': args.runs, 'baseline_runs': args.baseline_runs, 'baseline_chunk': args.baseline_chunk},
        'device': torch.cuda.get_device_name(0), 'src_sha': stamp.get('src_sha'),
    }
    line = json.dumps(result)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(result, indent=1) + '\n')
    print(line)


if __name__ == '__main__':
    main()
