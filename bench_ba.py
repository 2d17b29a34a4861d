#!/usr/bin/env python3
"""Timing of the scene-level bundle adjustment (cosypose_amd/bundle_adjustment.py) on one GPU: MultiviewRefinement.solve(n_iterations=100),
as MultiviewScenePredictor calls it, on a seeded synthetic scene (cosypose_amd.synthetic.make_ba_scene: by default 25 objects, 8 views,
200 points per object).  Prints one JSON line.  bench.py (the flagship workload) is a different script and is not affected.

    timeout -k 10 300 python bench_ba.py --seed 7 --warmup 2 --runs 5
"""
import argparse
import json
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seed', type=int, default=7)
    ap.add_argument('--objects', type=int, default=25)
    ap.add_argument('--views', type=int, default=8)
    ap.add_argument('--points', type=int, default=200)
    ap.add_argument('--iterations', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--runs', type=int, default=5)
    args = ap.parse_args()

    import torch
    from cosypose_amd import build, synthetic as syn
    from cosypose_amd.bundle_adjustment import MultiviewRefinement
    from cosypose_amd.mesh_db import BatchedMeshes
    assert torch.cuda.is_available(), 'bench_ba.py needs a ROCm device'
    scene = syn.make_ba_scene(args.seed, args.objects, args.views, args.points)
    problem = MultiviewRefinement(*syn.ba_scene_collections(scene, BatchedMeshes, device='cuda'))

    def solve():
        # host clock around synchronised ends: the loop reads the loss back after every linearisation, so host and device time of a solve
        # coincide; the events beside it confirm that (events_ms in the output)
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        start.record()
        out = problem.solve(n_iterations=args.iterations)
        end.record()
        torch.cuda.synchronize()
        out['events_ms'] = start.elapsed_time(end)
        return 1e3 * (time.perf_counter() - t0), out
    for _ in range(args.warmup):
        solve()
    runs = [solve() for _ in range(args.runs)]
    ms, out = min(runs, key=lambda r: r[0])
    h = out['history']
    n_hist = len(h['iteration'])
    n_lin = problem.n_linearisations

    def launch_ms(fn, reps=50):
        fn()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(reps):
            fn()
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end) / reps
    a, c = h['TWO_9d'][-1], h['TCW_9d'][-1]
    d = problem._device_state()
    split = dict(align=launch_ms(lambda: problem._align(a, c)))
    split['linearise'] = launch_ms(lambda: problem._linearize(a, c, 25)) - split['align']
    split['solve'] = launch_ms(lambda: problem._solve(1e-3))
    stamp = build.read_stamp() or {}
    print(json.dumps({
        'metric': 'bundle adjustment, MultiviewRefinement.solve (float64)', 'value': round(ms, 2), 'unit': 'ms/solve', 'higher_is_better': False,
        'runs_ms': [round(r[0], 2) for r in runs], 'events_ms': round(out['events_ms'], 2), 'time_init_ms': round(1e3 * out['time_init'], 2), 'time_opt_ms': round(1e3 * out['time_opt'], 2),
        'time_misc_ms': round(1e3 * out['time_misc'], 2), 'history_entries': n_hist, 'linearisations': n_lin,
        'ms_per_linearisation': round(1e3 * out['time_opt'] / n_lin, 3), 'launch_ms': {k: round(v, 4) for k, v in split.items()},
        'loss': [float(h['loss'][0]), float(h['loss'][-1])],
        'config': {'seed': args.seed, 'objects': problem.n_objects, 'views': problem.n_views, 'candidates': problem.n_candidates,
                   'points': d['P'], 'residuals': d['n_res'], 'unknowns': d['n'], 'n_iterations': args.iterations},
        'device': torch.cuda.get_device_name(0), 'src_sha': stamp.get('src_sha'),
        'ms_per_iteration': round(1e3 * out['time_opt'] / max(n_hist - 1, 1), 3),
        'cpu_reference': 'the reference on one CPU thread in float32 needs 0.73 s per ITERATION on a scene of this size (133 candidates; 72.7 s for the 100 '
                         'iterations it runs there, its stop rule never met): compare ms_per_iteration, not the whole solve, which stops early here',
    }))


if __name__ == '__main__':
    main()
