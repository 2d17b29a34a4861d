#!/usr/bin/env python3
"""Timing of the multi-view candidate matching (cosypose_amd/multiview_matching.py) on one GPU: multiview_candidate_matching with the
production setting n_ransac_iter=2000 on a seeded synthetic scene (cosypose_amd.synthetic.make_ba_scene with 8 box corners per mesh and
the true obj_id removed: by default 25 objects, 8 views, the size of bench_ba.py).  Prints one JSON line.  bench.py (the flagship
workload) is a different script and is not affected.

    timeout -k 10 300 python bench_ransac.py --seed 7 --warmup 3 --runs 30
"""
import argparse
import json
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seed', type=int, default=7)
    ap.add_argument('--objects', type=int, default=25)
    ap.add_argument('--views', type=int, default=8)
    ap.add_argument('--iterations', type=int, default=2000)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--runs', type=int, default=30)
    args = ap.parse_args()

    import numpy as np
    import torch
    from cosypose_amd import build, synthetic as syn, multiview_matching as mm
    from cosypose_amd.mesh_db import BatchedMeshes
    assert torch.cuda.is_available(), 'bench_ransac.py needs a ROCm device'
    scene = syn.make_ba_scene(args.seed, args.objects, args.views, 8)
    cand, _, _, mesh_db = syn.ba_scene_collections(scene, BatchedMeshes, dtype=torch.float32, device='cuda')
    cand.infos = cand.infos.drop(columns=['obj_id'])

    def run():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = mm.multiview_candidate_matching(cand, mesh_db, n_ransac_iter=args.iterations)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), out
    for _ in range(args.warmup):
        run()
    runs = [run() for _ in range(args.runs)]
    med = lambda v: float(np.median(v))
    out = runs[-1][1]

    # the host and device parts on their own
    view_ids, labels = cand.infos['view_id'].values, cand.infos['label'].values

    def host_ms(fn, reps=5):
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            r = fn()
            t.append(1e3 * (time.perf_counter() - t0))
        return med(t), r
    seed_ms, (seeds, tm) = host_ms(lambda: mm.make_ransac_infos(view_ids, labels, args.iterations, 0))
    scene_dev = mm._Scene(cand, mesh_db)
    plan_ms, plan = host_ms(lambda: mm._Plan(tm, scene_dev.device, scene_dev.n_cand))
    post_ms, _ = host_ms(lambda: (mm.scene_level_matching(cand, out['inliers']), mm.make_obj_infos(out['filtered_candidates'])))

    def launch_ms(fn, reps=200):
        fn()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(reps):
            fn()
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end) / reps
    table = torch.as_tensor(mm._seed_table(seeds, scene_dev.n_cand)).cuda()
    H = plan.H
    hyp = dict(TC1C2=torch.empty(H, 4, 4, device='cuda'), best=torch.empty(H, dtype=torch.int32, device='cuda'), gap=torch.empty(H, device='cuda'))
    lib, ptr, stream = mm.lib(), mm.ptr, mm.stream
    launches = dict(hypotheses=launch_ms(lambda: mm.check(lib.cosy_ransac_hypotheses(*scene_dev.args(True), ptr(table), H, ptr(hyp['TC1C2']),
                                                                                     ptr(hyp['best']), ptr(hyp['gap']), None, stream()))))
    n_inl = torch.empty(H, dtype=torch.int32, device='cuda')
    dsum = torch.empty(H, device='cuda')
    launches['score'] = launch_ms(lambda: mm.check(lib.cosy_ransac_score(
        *scene_dev.args(), ptr(hyp['TC1C2']), ptr(plan.hyp_pair), H, ptr(plan.pair_off), ptr(plan.tm), plan.n_pairs, plan.max_tm, 0.02,
        ptr(plan.hyp_dist_off), None, None, ptr(n_inl), ptr(dsum), stream())))
    best_hyp = torch.empty(plan.n_pairs, dtype=torch.int32, device='cuda')
    n_matches = torch.empty_like(best_hyp)
    match = torch.zeros(2, len(tm.pair_cand1), dtype=torch.int32, device='cuda')
    launches['best'] = launch_ms(lambda: mm.check(lib.cosy_ransac_best(
        *scene_dev.args(), ptr(hyp['TC1C2']), H, ptr(n_inl), ptr(dsum), ptr(plan.pair_hyp_off), ptr(plan.pair_hyps), ptr(plan.pair_off), ptr(plan.tm),
        plan.n_pairs, plan.max_tm, 0.02, 3, 1, ptr(plan.hyp_dist_off), None, ptr(best_hyp), ptr(n_matches), ptr(match[0]), ptr(match[1]), stream())))
    device_ms = sum(launches.values())
    # float32 operations one scoring needs (multiplies and adds counted apiece: the kernels are compiled with contraction off, so
    # each is an instruction): TC1C2 TC2Ob, then per symmetry TC1Oa S and per point two transforms, the difference, its square norm
    # and root, two accumulations
    S, P = scene_dev.S, scene_dev.P
    flop_per_scoring = 128 + S * (128 + P * (2 * 18 + 3 + 5 + 1 + 2))
    score_tflops = plan.n_scorings * flop_per_scoring / (1e-3 * launches['score']) / 1e12

    matched = out['filtered_candidates']
    truth = scene['cand_obj_id'][matched.infos['cand_id'].values]
    groups = lambda ids: sorted(tuple(np.flatnonzero(ids == i)) for i in set(ids.tolist()))
    stamp = build.read_stamp() or {}
    ms = med([r[0] for r in runs])
    print(json.dumps({
        'metric': 'multi-view candidate matching, multiview_candidate_matching (float32)', 'value': round(ms, 2), 'unit': 'ms/call', 'higher_is_better': False,
        'runs_ms': [round(r[0], 2) for r in runs],
        'time_models_ms': round(1e3 * med([r[1]['time_models'] for r in runs]), 3), 'time_score_ms': round(1e3 * med([r[1]['time_score'] for r in runs]), 3),
        'time_misc_ms': round(1e3 * med([r[1]['time_misc'] for r in runs]), 3),
        'launch_ms': {k: round(v, 4) for k, v in launches.items()}, 'device_ms': round(device_ms, 4),
        'host_ms': {'make_ransac_infos': round(seed_ms, 3), 'id_tables_and_upload': round(plan_ms, 3), 'components_and_frames': round(post_ms, 3)},
        'hypotheses': H, 'scorings': plan.n_scorings, 'hypotheses_per_s': round(H / (1e-3 * launches['hypotheses'])),
        'scorings_per_s': round(plan.n_scorings / (1e-3 * launches['score'])), 'scorings_per_s_whole_call': round(plan.n_scorings / (1e-3 * ms)),
        'score_launch': {'flop_per_scoring': flop_per_scoring, 'tflops': round(score_tflops, 2),
                         'share_of_fp32_vector_peak': round(score_tflops / 78.65, 3),
                         'peak': '78.65 T instructions/s: 157.3 TFLOPS counts a fused multiply-add as two, these kernels issue none'},
        'config': {'seed': args.seed, 'objects': args.objects, 'views': args.views, 'candidates': len(cand), 'n_ransac_iter': args.iterations,
                   'view_pairs': plan.n_pairs, 'longest_tmatch_list': plan.max_tm},
        'result': {'view_pairs': len(out['pairs_TC1C2']), 'objects': len(out['scene_infos']), 'candidates_kept': len(matched),
                   'partition_is_ground_truth': groups(matched.infos['obj_id'].values) == groups(truth)},
        'device': torch.cuda.get_device_name(0), 'src_sha': stamp.get('src_sha'),
        'cpu_reference': 'the reference on one CPU thread in float32 with its compiled cosypose_cext needs 81 s for the default scene (seed 7, 25 objects, '
                         '8 views: 157 candidates, 112,000 hypotheses, 12,452,000 scorings), 77 s of it scoring',
    }))


if __name__ == '__main__':
    main()
