#!/usr/bin/env python3
"""Timing of the pose-evaluation errors (cosypose_amd.distances.pose_errors, csrc/kernels_eval.hip) on one GPU, on an evaluation-sized
workload: 4096 tentative (prediction, ground truth) pairs of 21 objects whose meshes hold 2 000 - 40 000 points (log-uniform), ADD(-S)
with every second object symmetric.  Prints one JSON line.  bench.py (the flagship workload) is a different script and is not affected.

    timeout -k 10 600 python bench_eval.py --warmup 1 --runs 5 --out profiles/eval_bench.json

Reported: milliseconds per pose_errors call (median of the runs, device events, all in this process), pairs of points per second, the
same pairs through the route the package offered before -- dists_add_symmetric / dists_add per pair plus torch reductions, which is
what the reference's errors_bsz = 1 loop amounts to -- and the VALU-issue time of the ADD-S inner loop: instructions per point pair
counted in the shipped kernel's assembly (profiles/eval_isa.json, written by profiles/exp/eval_isa_count.py) over 256 CUs x 4 SIMDs at
the device's clock, priced twice: at 3.1 cycles per wave instruction (`valu_floor_ms`: the v_fma_f32 / v_mul_f32 figure measured by
profiles/exp/valu_bench.hip at 4 or more waves per SIMD) and at 2 cycles (`issue_limit_ms`: 64 lanes on a 32-lane SIMD, the rate no
instruction stream can beat).  `achieved_cycles_per_wave_instruction` is the call's whole time over the loop's instructions.
`gate_ok`: the fused call is not slower than the per-pair route by more than the run-to-run spread.
"""
import argparse
import hashlib
import json
import os
import statistics

HERE = os.path.dirname(os.path.abspath(__file__))
VALU_CYCLES = 3.1        # per wave instruction, profiles/exp/valu_bench.hip


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seed', type=int, default=3)
    ap.add_argument('--pairs', type=int, default=4096)
    ap.add_argument('--objects', type=int, default=21)
    ap.add_argument('--min-points', type=int, default=2000)
    ap.add_argument('--max-points', type=int, default=40000)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--baseline-runs', type=int, default=3)
    ap.add_argument('--out', default=None, help='also write the result to this JSON file')
    args = ap.parse_args()

    import numpy as np
    import torch
    from cosypose_amd import build, distances, synthetic as syn
    assert torch.cuda.is_available(), 'bench_eval.py needs a ROCm device'
    rs = np.random.RandomState(args.seed)
    n_points = np.exp(rs.uniform(np.log(args.min_points), np.log(args.max_points), args.objects)).astype(np.int32)
    n_points[0], n_points[-1] = args.min_points, args.max_points
    symmetric = (np.arange(args.objects) % 2).astype(np.int32)
    table = np.zeros((args.objects, int(n_points.max()), 3), np.float32)
    for o, P in enumerate(n_points):
        table[o, :P] = rs.uniform(-1, 1, (P, 3)) * rs.uniform(0.03, 0.12, 3)
    obj = rs.randint(0, args.objects, args.pairs).astype(np.int32)
    mode = symmetric[obj]
    TXO_gt = syn.make_TCO(args.seed + 1, args.pairs)
    noise = np.stack([syn._rigid_noise(rs, 0.05, 0.01) for _ in range(args.pairs)])
    TXO_pred = (TXO_gt.astype(np.float64) @ noise).astype(np.float32)
    d = lambda a: torch.from_numpy(a).cuda()
    table_d, pred_d, gt_d, obj_d, mode_d, n_d = d(table), d(TXO_pred), d(TXO_gt), d(obj), d(mode), d(n_points)
    point_pairs = float(sum(float(n_points[o]) ** 2 if symmetric[o] else float(n_points[o]) for o in obj))

    def timed(fn):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        out = fn()
        end.record()
        torch.cuda.synchronize()
        return start.elapsed_time(end), out

    fused = lambda: distances.pose_errors(pred_d, gt_d, obj_d, mode_d, table_d, n_d)

    def per_pair():
        """errors_bsz = 1: one dists_add / dists_add_symmetric call per pair on its object's own points, reduced by torch"""
        norm = torch.empty(args.pairs, device='cuda')
        xyz = torch.empty(args.pairs, 3, device='cuda')
        for b in range(args.pairs):
            pts = table_d[obj[b], :n_points[obj[b]]][None]
            fn = distances.dists_add_symmetric if mode[b] else distances.dists_add
            dists = fn(pred_d[b:b + 1], gt_d[b:b + 1], pts)
            norm[b] = torch.norm(dists, dim=-1, p=2).mean(-1)[0]
            xyz[b] = dists.abs().mean(dim=-2)[0]
        return dict(norm_avg=norm, xyz_avg=xyz)

    for _ in range(args.warmup):
        fused()
    runs = [timed(fused) for _ in range(args.runs)]
    if args.warmup:
        per_pair()
    base = [timed(per_pair) for _ in range(args.baseline_runs)]
    ms, base_ms = statistics.median(r[0] for r in runs), statistics.median(r[0] for r in base)
    spread = max(max(r[0] for r in runs) - min(r[0] for r in runs), max(r[0] for r in base) - min(r[0] for r in base))
    a, b = runs[-1][1], base[-1][1]
    agree = float(((a['norm_avg'] - b['norm_avg']).abs() / b['norm_avg']).max())

    isa_path = os.path.join(HERE, 'profiles', 'eval_isa.json')
    isa = json.load(open(isa_path)) if os.path.exists(isa_path) else None
    src = os.path.join(HERE, 'cosypose_amd', 'csrc', 'kernels_eval.hip')
    if isa and os.path.exists(src) and hashlib.sha256(open(src, 'rb').read()).hexdigest()[:16] != isa['src_sha']:
        isa = None                                                  # counted on another version of the kernel
    props = torch.cuda.get_device_properties(0)
    clock_ghz = getattr(props, 'clock_rate', 2400000) / 1e6
    floor_ms = limit_ms = achieved = None
    if isa:
        sym_pairs = float(sum(float(n_points[o]) ** 2 for o in obj if symmetric[o]))
        wave_instructions = sym_pairs * isa['valu_per_pair'] / 64
        simd_hz = props.multi_processor_count * 4 * clock_ghz * 1e9
        floor_ms, limit_ms = 1e3 * wave_instructions * VALU_CYCLES / simd_hz, 1e3 * wave_instructions * 2 / simd_hz
        achieved = ms * 1e-3 * simd_hz / wave_instructions
    stamp = build.read_stamp() or {}
    result = {
        'metric': 'pose evaluation errors, distances.pose_errors (ADD(-S), one call)', 'value': round(ms, 3), 'unit': 'ms/call', 'higher_is_better': False,
        'runs_ms': [round(r[0], 3) for r in runs], 'point_pairs': point_pairs, 'point_pairs_per_s': round(point_pairs / (ms * 1e-3), 1),
        'per_pair_route_ms': round(base_ms, 3), 'per_pair_route_runs_ms': [round(r[0], 3) for r in base], 'speedup_vs_per_pair_route': round(base_ms / ms, 3),
        'run_to_run_spread_ms': round(spread, 3), 'gate_ok': bool(ms <= base_ms + spread), 'max_rel_diff_norm_avg_vs_per_pair_route': agree,
        'valu_floor_ms': None if floor_ms is None else round(floor_ms, 3), 'fraction_of_valu_floor': None if floor_ms is None else round(floor_ms / ms, 4),
        'issue_limit_ms': None if limit_ms is None else round(limit_ms, 3), 'fraction_of_issue_limit': None if limit_ms is None else round(limit_ms / ms, 4),
        'achieved_cycles_per_wave_instruction': None if achieved is None else round(achieved, 3),
        'valu_per_point_pair': isa and isa['valu_per_pair'], 'valu_cycles_per_wave_instruction': VALU_CYCLES, 'clock_ghz': clock_ghz,
        'compute_units': props.multi_processor_count,
        'config': {'seed': args.seed, 'pairs': args.pairs, 'objects': args.objects, 'n_points': [int(n) for n in n_points],
                   'symmetric_pairs': int(mode.sum()), 'warmup': args.warmup, 'runs': args.runs, 'baseline_runs': args.baseline_runs},
        'device': torch.cuda.get_device_name(0), 'src_sha': stamp.get('src_sha'),
    }
    line = json.dumps(result)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(result, indent=1) + '\n')
    print(line)


if __name__ == '__main__':
    main()
