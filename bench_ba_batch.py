#!/usr/bin/env python3
"""Timing of the batched bundle adjustment (cosypose_amd.bundle_adjustment.solve_problems) on one GPU against the per-problem loop
beside it: G sub-problems (default 64) of ONE seeded synthetic scene (cosypose_amd.synthetic.make_ba_scene, 25 objects, 8 views, 200
points per object), each with 4-8 of its views and 4-10 of its objects, n_iterations=100 as MultiviewScenePredictor calls it.
Prints one JSON line: ms of one solve_problems call, ms of `for p in problems: p.solve()` in the same process (the path that
predict_scene_state takes), their ratio, the batch's launches timed one by one, and the number of host reads.  bench.py (the flagship
workload) is a different script and is not affected.

    timeout -k 10 300 python bench_ba_batch.py --seed 7 --warmup 2 --runs 5
"""
import argparse
import ctypes
import json
import time


def make_problems(args, device='cuda'):
    import numpy as np
    from cosypose_amd import synthetic as syn
    from cosypose_amd.bundle_adjustment import MultiviewRefinement
    from cosypose_amd.mesh_db import BatchedMeshes
    scene = syn.make_ba_scene(args.seed, args.objects, args.views, args.points)
    mesh_db = syn.ba_scene_collections(scene, BatchedMeshes, device=device)[3]
    rs = np.random.RandomState(args.seed)
    obj_ids = np.unique(scene['cand_obj_id'])
    problems = []
    while len(problems) < args.problems:
        views = scene['cam_view_id'][rs.choice(args.views, rs.randint(4, 9), replace=False)]
        objects = obj_ids[rs.choice(len(obj_ids), rs.randint(4, 11), replace=False)]
        cand = np.isin(scene['cand_view_id'], views) & np.isin(scene['cand_obj_id'], objects)
        if len(np.unique(scene['cand_view_id'][cand])) < 4 or len(np.unique(scene['cand_obj_id'][cand])) < 4:
            continue        # a drawn view that sees none of the drawn objects would drop out of the problem
        sub = dict(scene)
        sub.update({k: v[cand] for k, v in scene.items() if k.startswith('cand_')})
        problems.append(MultiviewRefinement(*syn.ba_scene_collections(sub, lambda *a: mesh_db, device=device)))
    return problems


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seed', type=int, default=7)
    ap.add_argument('--problems', type=int, default=64)
    ap.add_argument('--objects', type=int, default=25)
    ap.add_argument('--views', type=int, default=8)
    ap.add_argument('--points', type=int, default=200)
    ap.add_argument('--iterations', type=int, default=100)
    ap.add_argument('--poll-every', type=int, default=8)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--runs', type=int, default=5)
    args = ap.parse_args()

    import torch
    from cosypose_amd import build, bundle_adjustment as ba
    from cosypose_amd._lib import lib, check, stream
    assert torch.cuda.is_available(), 'bench_ba_batch.py needs a ROCm device'
    problems = make_problems(args)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), out
    batched = lambda: ba.solve_problems(problems, n_iterations=args.iterations, history=False, poll_every=args.poll_every)
    loop = lambda: [p.solve(n_iterations=args.iterations) for p in problems]
    for _ in range(args.warmup):
        batched(), loop()
    runs_b = [timed(batched) for _ in range(args.runs)]
    runs_l = [timed(loop) for _ in range(args.runs)]
    ms_b, out_b = min(runs_b, key=lambda r: r[0])
    ms_l, out_l = min(runs_l, key=lambda r: r[0])
    same = all(a['history']['lambda'] == b['history']['lambda'] and torch.equal(torch.stack(a['history']['loss']), torch.stack(b['history']['loss']))
               for a, b in zip(out_b, out_l))
    entries = [len(o['history']['iteration']) for o in out_b]

    # the batch's launches one by one, every problem active (fresh control records)
    plan = ba._batch_plan(problems)
    starts = [p.robust_initialization_TWO_TCW() for p in problems]
    b = ba._Batch(problems, plan, torch.cat([a for a, _ in starts]), torch.cat([c for _, c in starts]), True, args.iterations, 25, 1e-3, 9, 11, 1e-5,
                  False)
    cb, l = ctypes.addressof(b.c), lib()

    def launch_ms(fn, reps=20):
        fn()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(reps):
            fn()
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end) / reps
    split = dict(linearise=launch_ms(lambda: check(l.cosy_ba_batch_linearize(cb, 1, stream()))))
    check(l.cosy_ba_batch_linearize(cb, 0, stream()))
    split['solve_step'] = launch_ms(lambda: check(l.cosy_ba_batch_solve_step(cb, stream())))
    split['decide'] = launch_ms(lambda: check(l.cosy_ba_batch_decide(b.c.ctrl, b.c.G, 9., 11., 1e-5, None, 0, 0, None, None, None, None, stream())))
    b2 = ba._Batch(problems, plan, b.TWO, b.TCW, True, 64, 25, 1e-3, 9, 11, 1e-5, False)
    n = [0]

    def record():
        check(l.cosy_ba_batch_record(b2.c.ctrl, b2.c.G, n[0], 64, None, 0, 0, 0, None, None, b2.c.hist_iteration, b2.c.hist_lambda, b2.c.hist_loss,
                                     None, None, stream()))
        n[0] += 1
    split['record'] = launch_ms(record)
    split['iteration'] = 2 * split['linearise'] + split['solve_step'] + split['decide'] + split['record']
    stamp = build.read_stamp() or {}
    print(json.dumps({
        'metric': 'batched bundle adjustment, solve_problems (float64)', 'value': round(ms_b, 2), 'unit': 'ms/batch', 'higher_is_better': False,
        'loop_ms': round(ms_l, 2), 'loop_over_batched': round(ms_l / ms_b, 2), 'runs_batched_ms': [round(r[0], 2) for r in runs_b],
        'runs_loop_ms': [round(r[0], 2) for r in runs_l], 'n_host_reads': out_b[0]['n_host_reads'],
        'iterations_launched': out_b[0]['n_iterations_launched'], 'time_init_ms': round(1e3 * out_b[0]['time_init'], 2),
        'time_opt_ms': round(1e3 * out_b[0]['time_opt'], 2), 'time_misc_ms': round(1e3 * out_b[0]['time_misc'], 2),
        'launch_ms': {k: round(v, 4) for k, v in split.items()}, 'history_entries': {'min': min(entries), 'max': max(entries), 'sum': sum(entries)},
        'same_bits_as_loop': same,
        'config': {'seed': args.seed, 'problems': len(problems), 'views': [min(p.n_views for p in problems), max(p.n_views for p in problems)],
                   'objects': [min(p.n_objects for p in problems), max(p.n_objects for p in problems)],
                   'candidates': sum(p.n_candidates for p in problems), 'points': args.points, 'unknowns_max': int(plan['n'].max()),
                   'n_iterations': args.iterations, 'poll_every': args.poll_every},
        'device': torch.cuda.get_device_name(0), 'src_sha': stamp.get('src_sha'),
    }))


if __name__ == '__main__':
    main()
