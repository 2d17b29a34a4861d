#!/usr/bin/env python3
"""Timing of the object-model pass (cosypose_amd.model_info, csrc/kernels_models.hip) on one GPU: 30 synthetic models of 2 000 to 40 000
vertices (the size range of bench_bop.py's meshes), float32 vertices in millimetres, all in ONE call -- diameters, boxes and the
non-finite counts.  Prints one JSON line.  bench.py (the flagship workload) is a different script and is not affected.

    timeout -k 10 600 python bench_models.py --warmup 1 --runs 5 --out profiles/models_bench.json

Reported: milliseconds per model_info call (median of the runs, device events, all in this process; the upload of the offsets and the one
device-to-host copy of the records inside the timed region) and the same diameters through what torch offers on the device: torch.cdist
in float64 (its default route, |a|^2 + |b|^2 - 2 a.b through a matrix product), in row chunks, followed by max -- it writes 8 bytes per
pair to memory, the kernel keeps its tiles on chip.  (compute_mode='donot_use_mm_for_euclid_dist' is not the baseline: at these sizes it
returned diameters that were plainly wrong on the MI355X -- larger than the true maximum, and the same value for two different models.)  `gate_ok`: the kernel is not slower than that route by more than the run-to-run spread.  Where SciPy is installed, cdist on
one CPU core is timed on the SMALLEST model only and scaled by the pair count to the whole set: `scipy_one_core_ms_scaled` is an
extrapolation, labelled as such.  Before anything is timed the kernel's diameter of the smallest model is compared bit for bit with a
NumPy float64 restatement (and with SciPy's cdist where installed), and the torch route's diameters must agree with the kernel's to
1e-12 relative: the matrix form rounds differently, so its last bits are its own.
"""
import argparse
import json
import statistics
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seed', type=int, default=7)
    ap.add_argument('--models', type=int, default=30)
    ap.add_argument('--v-min', type=int, default=2000)
    ap.add_argument('--v-max', type=int, default=40000)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--baseline-runs', type=int, default=3)
    ap.add_argument('--baseline-chunk-mib', type=int, default=256, help='size of one float64 distance block of the torch route')
    ap.add_argument('--out', default=None, help='also write the result to this JSON file')
    args = ap.parse_args()

    import numpy as np
    import torch
    from cosypose_amd import build, model_info
    assert torch.cuda.is_available(), 'bench_models.py needs a ROCm device'
    rs = np.random.RandomState(args.seed)
    sizes = np.linspace(args.v_min, args.v_max, args.models).round().astype(int)
    # bumpy ellipsoids of some 100 mm: many vertices near the hull, as a scanned object has
    models = []
    for V in sizes:
        d = rs.standard_normal((V, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        models.append(np.ascontiguousarray((d * rs.uniform(40, 120, 3) * (1 + 0.05 * rs.standard_normal((V, 1)))).astype(np.float32)))
    verts = [torch.from_numpy(p).cuda() for p in models]
    pairs = int(sum(int(V) * (int(V) - 1) // 2 for V in sizes))

    def event():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def fused():
        torch.cuda.synchronize()
        e0 = event()
        out = model_info(verts)
        e1 = event()
        torch.cuda.synchronize()
        return dict(ms=e0.elapsed_time(e1), out=np.array([m['diameter'] for m in out]))

    rows_per_chunk = lambda V: max(1, (args.baseline_chunk_mib << 20) // (8 * int(V)))

    def torch_route():
        """float64 cdist in row chunks, then max; one device-to-host copy at the end, as the fused call has"""
        torch.cuda.synchronize()
        e0 = event()
        best = []
        for p in verts:
            q = p.double()
            step = rows_per_chunk(len(q))
            best.append(torch.stack([torch.cdist(q[lo:lo + step], q).max()
                                     for lo in range(0, len(q), step)]).max())
        out = torch.stack(best).cpu().numpy()
        e1 = event()
        torch.cuda.synchronize()
        return dict(ms=e0.elapsed_time(e1), out=out)

    # ---- equal diameters before anything is timed
    a, b = fused()['out'], torch_route()['out']
    p0 = models[0].astype(np.float64)
    d = p0[:, None, :] - p0[None, :, :]
    numpy_d0 = np.sqrt(((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).max())      # one rounding per operation
    assert a[0] == numpy_d0, (a[0], numpy_d0)                                    # the contract: these bits
    rel = np.abs(a - b) / a                                                      # the matrix form rounds differently: its last bits are its own
    assert rel.max() <= 1e-12, (a, b)
    equal_torch = int((a == b).sum())
    scipy_ms = scipy_equal = None
    try:
        from scipy.spatial.distance import cdist
        t0 = time.perf_counter()
        d0 = cdist(p0, p0).max()
        scipy_small_ms = (time.perf_counter() - t0) * 1e3
        scipy_equal = bool(d0 == a[0])
        assert scipy_equal, (d0, a[0])
        scipy_ms = scipy_small_ms * (sum(float(V) ** 2 for V in sizes) / float(sizes[0]) ** 2)
    except ImportError:
        pass

    for _ in range(args.warmup):
        fused()
    runs = [fused() for _ in range(args.runs)]
    if args.warmup:
        torch_route()
    base = [torch_route() for _ in range(args.baseline_runs)]
    med = lambda rows, k: statistics.median(r[k] for r in rows)
    ms, base_ms = med(runs, 'ms'), med(base, 'ms')
    spread = max(max(r['ms'] for r in runs) - min(r['ms'] for r in runs), max(r['ms'] for r in base) - min(r['ms'] for r in base))
    stamp = build.read_stamp() or {}
    result = {
        'metric': 'object models, model_info (diameter, box, non-finite count of every model, one call)', 'value': round(ms, 3), 'unit': 'ms/call',
        'higher_is_better': False, 'runs_ms': [round(r['ms'], 3) for r in runs],
        'torch_cdist_f64_ms': round(base_ms, 3), 'torch_cdist_f64_runs_ms': [round(r['ms'], 3) for r in base],
        'speedup_vs_torch_cdist_f64': round(base_ms / ms, 3), 'run_to_run_spread_ms': round(spread, 3), 'gate_ok': bool(ms <= base_ms + spread),
        'vertex_pairs': pairs, 'gpairs_per_s': round(pairs / ms * 1e-6, 2),
        'diameter_equal_numpy_f64_bitwise_smallest_model': True, 'diameters_equal_torch_bitwise': f'{equal_torch} of {len(sizes)}',
        'max_rel_difference_from_torch': float(rel.max()),
        'diameter_equal_scipy_bitwise_smallest_model': scipy_equal,
        'scipy_one_core_ms_scaled': None if scipy_ms is None else round(scipy_ms, 1),
        'scipy_note': None if scipy_ms is None else f'cdist + max of the {int(sizes[0])}-vertex model on one core, SCALED by the sum of V^2; not measured on the set',
        'config': {'seed': args.seed, 'models': int(len(sizes)), 'v_min': int(sizes[0]), 'v_max': int(sizes[-1]), 'vertices': int(sizes.sum()),
                   'dtype': 'float32', 'warmup': args.warmup, 'runs': args.runs, 'baseline_runs': args.baseline_runs,
                   'baseline_chunk_mib': args.baseline_chunk_mib},
        'device': torch.cuda.get_device_name(0), 'src_sha': stamp.get('src_sha'),
    }
    line = json.dumps(result)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(json.dumps(result, indent=1) + '\n')
    print(line)


if __name__ == '__main__':
    main()
