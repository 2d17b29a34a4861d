#!/usr/bin/env python3
"""Headline benchmark: refined pose-iterations/sec of the render-and-compare hot path on MI355X.

A "step" = one pass of the hot path over one batch of synthetic input.  --config selects the BASELINE.json workload:
  1 (default, the metric's config): D=256 detections per GPU over 16 frames 512x512, 21 objects, coarse 1 + refiner 4
    iterations = 1280 pose-iterations per GPU per step, 256x256 crops, 16-bit backbone; weak scaling (each rank its own 256);
  2: T-LESS shape: 1024 candidates over 64 frames 540x720, 30 objects, refiner-only 4 iterations from given poses, fp16;
     STRONG scaling: the 1024 candidates are sharded over the ranks (get_predictions_sharded);
  3: BOP mix: 2048 candidates over 7 frame sizes (5x 640x480, 720x540, 1280x960), coarse 1 + refiner 4, bf16, strong
     scaling with --split skewed (per-rank shares ~ [512,384,320,256,224,160,128,64]/2048) or balanced (equal counts).
Everything (frames, intrinsics, detections, mesh table, weights, the synthetic renderer's images) is resident in HBM
before the timed region.  The refined poses of all ranks are exchanged by ONE RCCL all-gather per step.
Schedule inside a rank: the candidates are cut into --streams (default 2) equal chunks that each run coarse -> refiner on their own
HIP stream (CoarseRefinePosePredictor n_streams; results bit-identical to one stream, tests/test_gpu_parity.py): another chunk's
kernels fill the ramp-up / drain of each of the ~90 dependent launches of a forward.  `config.single_stream` is the same workload as
ONE stream of full-size launches (the schedule of the earlier rounds' lines), timed in the same process.

Storage type.  BASELINE configs[1] names bf16 AND north_star demands <= 1e-4 relative pose deviation; measured, bf16 storage
(8 significant bits on every stored activation and weight) cannot meet that bound (3-6e-4 per parameter group) while fp16
(11 bits, same bytes, same MFMA rate, saturating converts) does (<= 5e-5).  Parity is the first gate, so the headline
`value` is measured in fp16; the same timed loop is repeated in bf16 and fp32 and reported beside it (`other_dtypes`), and
`pose_deviation` is measured live: the benched dtype's refined poses against the fp32 HIP path (itself held to the reference
at <= 1e-4 by the parity tests) on this very workload, per parameter group (rotation entries absolute, translation relative
to each pose's own translation), and -- `pose_deviation.vs_oracle`, inside the cpu_baseline leg -- against the CPU ORACLE on the
first 32 detections of the workload through all five iterations, for every benched storage type.

A plain run (`bench.py --gpus 1 --steps N --warmup W`) does only what the headline needs: set-up, W warm-up steps, the N timed steps,
the outputs of the last timed step when --dump-outputs DIR is given, and the JSON line.  Everything else below -- the single-stream
schedule, the collective alone, `roofline`, `other_dtypes`, `pose_deviation` and `cpu_baseline` -- is measured only with --full (--layers
implies it); their fields are null otherwise, and --no-cpu-baseline / --no-other-dtypes / --no-profile drop parts of it.
--dump-outputs DIR writes, after the timed steps, what the last timed step returned (rank 0): the refined poses of all candidates
(`poses.npy`) and, where the path returns them, every stage / iteration's result tensors (`<stage>_iteration<k>_<field>.npy`), float32,
at most 64 MB together (larger outputs: a fixed, seeded sample of rows).  The inputs depend on the arguments alone, so two builds can be
compared output for output.

One JSON line on stdout (rank 0).  `roofline` is for the dominant kernel FAMILY of the backbone (all instantiations of one
kernel template together; the dominant single instantiation and the next two are reported beside it), timed live with HIP events recorded on
the launch stream after every launch (cosy_effnet_b3_set_profiling) in a second pass over the same steps right after the
timed region (an event per kernel costs ~6 % of throughput, so not inside it).  `roofline.traffic` (HBM bytes per launch
from PMC counters) cannot be measured from inside this process: it is taken from the newest profiles/r*_pmc_traffic.json ONLY when
that file was collected for the same kernel sources (its `csrc_sha` matches the tree); otherwise null.
`cpu_baseline` is the CPU oracle (a port of the reference's PyTorch-CPU arithmetic) on a bounded sample: warm-up, then the
median of 5 repeats, at 1 thread (the reference pins OMP_NUM_THREADS=1) and at N threads.
"""
import argparse
import gc
import hashlib
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

HBM_PEAK_GBS = 8000.0        # MI355X HBM3E spec (MI355X_MICROARCH.md: 8.0 TB/s spec, ~6.3 achievable)
MFMA_PEAK_TFLOPS = {'bf16': 2500.0, 'fp16': 2500.0, 'fp32': 157.3}
ALGO_MB_PER_POSE_ITER = {('bf16', 256): 10.7, ('fp16', 256): 10.7, ('fp32', 256): 21.3, ('bf16', 240): 12.4, ('fp16', 240): 12.4, ('fp32', 240): 24.9}
SKEW = [512, 384, 320, 256, 224, 160, 128, 64]
DEFAULT_STREAMS = 2     # chunks of a rank on two HIP streams (CoarseRefinePosePredictor n_streams): +3.5 % at the headline workload, bit-identical results
NAMED_DTYPE = {1: 'bf16', 2: 'fp16', 3: 'bf16'}     # the storage type BASELINE.json's configs[i] names (3: the docstring's choice)


# VALU issue costs measured on MI355X (profiles/exp/valu_bench.hip, >= 4 waves per SIMD), cycles per wave64 instruction
VALU_CYC = dict(fma=3.1, trans=8.7, cvt_pk=4.7)
GPU_CLOCK_GHZ, N_SIMD = 2.4, 1024


def valu_bound(name, k, batch, crop, front_kind=None):
    """Issue-slot floor of a fused-front launch (mbconv_wave_kernel / mbconv_small_kernel / mbconv_small_mx_kernel): these kernels are bound by
    the vector ALU beside the matrix cores, not by HBM or MFMA, so the line prices them against THAT roof too.  Model, per 64
    elements: BN + SiLU = fma + (exp, rcp) + add + mul = 3 x 3.1 + 2 x 8.7 = 26.7 cycles, once per EXPANDED element (S^2 per
    output element) and once per output element; one squeeze add and half a packed convert per output element; then either k^2 tap FMAs
    (fp32-FMA form) or, where the taps run on the matrix pipe (round 5: stride-1 wave variants on full 16-pixel segments, the 8x8-map kernel),
    what feeds the small MFMAs instead: the expanded value's clamp + half a packed convert, one lane move / select per output, the output's clamp
    and the conversion back behind the transposing MFMA.  floor = instruction-cycles / (1024 SIMDs x 2.4 GHz); `frac` = floor / measured launch time."""
    import re
    from cosypose_amd import arch
    m = re.match(r'mbconv_(wave|small|small_mx)_kernel<([^,]+), (\d)(?:, (\d))?', name)
    if not m:
        return None
    ks, st = int(m.group(3)), (int(m.group(4)) if m.group(1) != 'small_mx' and m.group(4) else 1)
    # which form of the depthwise the launches ran comes from the engine itself (cosy_effnet_b3_block_info: front kinds 5 / 6 = taps on the matrix
    # pipe), not from a re-derivation of kernels_wave.hip's predicate on the kernel name
    kinds = {front_kind.get(l) for l in k['layers']} if front_kind else set()
    mx = bool(kinds) and kinds <= {5, 6}
    silu = 3 * VALU_CYC['fma'] + 2 * VALU_CYC['trans']
    per_out = st * st * silu + silu + VALU_CYC['cvt_pk'] / 2 + VALU_CYC['fma']
    per_out += (2 * VALU_CYC['fma'] + VALU_CYC['cvt_pk'] + VALU_CYC['fma']) if mx else ks * ks * VALU_CYC['fma']
    h, w = arch.conv_out(crop[0], 3, 2), arch.conv_out(crop[1], 3, 2)
    elems, n_layers = 0.0, 0
    for i, (bk, bs, e, cin, cout) in enumerate(arch.B3_BLOCKS):
        ho, wo = arch.conv_out(h, bk, bs), arch.conv_out(w, bk, bs)
        if i in k['layers']:
            elems += float(batch) * ho * wo * cin * e
            n_layers += 1
        h, w = ho, wo
    if not n_layers:
        return None
    floor_us = elems / n_layers / 64.0 * per_out / (N_SIMD * GPU_CLOCK_GHZ * 1e3)
    return dict(floor_us=round(floor_us, 1), frac=round(floor_us / (k['ms'] / k['n'] * 1e3), 3), cycles_per_64_outputs=round(per_out, 1),
                taps='matrix pipe' if mx else 'fp32 FMA',
                model='issue cycles of BN+SiLU on the expanded and the output elements, k*k tap FMAs (or the conversions and lane moves that feed the tap MFMAs), convert, squeeze add at the measured '
                      'per-instruction costs (fma 3.1, exp / rcp 8.7, cvt_pk 4.7 cycles per wave64 instruction), 1024 SIMDs at 2.4 GHz')


class SyntheticRenderer:
    """Stand-in for renderer.render (out of scope): returns pre-generated device images."""

    def __init__(self, renders):
        self.renders, self.i = renders, 0

    def render(self, obj_infos, TCO, K, resolution):
        r = self.renders[self.i % len(self.renders)]
        self.i += 1
        return r[:len(obj_infos)]


def build_model(seed, mesh_db, render_size, dtype, renderer):
    import argparse as ap
    import torch
    from cosypose_amd import synthetic as syn
    from cosypose_amd.pose_models_cfg import create_model_pose, check_update_config
    cfg = check_update_config(ap.Namespace(backbone_str='efficientnet-b3', n_pose_dims=9))
    m = create_model_pose(cfg, renderer, mesh_db)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in syn.golden_state_dict(seed).items()}, strict=False)
    m.cfg = cfg
    m.render_size = render_size
    m.compute_dtype = dtype
    return m.cuda().eval()


def csrc_sha():
    h = hashlib.sha256()
    d = os.path.join(REPO, 'cosypose_amd', 'csrc')
    for f in sorted(os.listdir(d)):
        h.update(f.encode()); h.update(open(os.path.join(d, f), 'rb').read())
    return h.hexdigest()[:16]


def host_cpu():
    model = ''
    try:
        for ln in open('/proc/cpuinfo'):
            if ln.startswith('model name'):
                model = ln.split(':', 1)[1].strip(); break
    except OSError:
        pass
    return model, os.cpu_count() or 1


def _cpu_worker(args):
    """one process of the all-cores CPU baseline: `n_det` detections per call at `threads` threads, pinned to the logical CPUs `cpus` (None: unpinned),
    `calls` timed calls after a warm-up"""
    H, W, threads, calls, seed, n_det, cpus = args
    if cpus:
        try:
            os.sched_setaffinity(0, cpus)
        except (AttributeError, OSError):
            pass
    os.environ['OMP_NUM_THREADS'] = str(threads)
    sys.path.insert(0, os.path.join(REPO, 'oracle'))
    import torch
    import cosy_oracle as O
    from cosypose_amd import synthetic as syn
    torch.set_num_threads(threads); O.set_threads(threads)
    tr = O.TorchRef(syn.golden_state_dict(0))
    pts = syn.make_mesh_points(7, 21, 2500)[:, np.random.RandomState(0).choice(2500, 2000, replace=False)]
    h, w = (512, 512) if H == W else (480, 640)
    obj, im, boxes = syn.make_detections(1 + seed, n_det, 2, 21, h, w)
    frames = syn.make_frames(2, 2, h, w)[im]
    K = syn.make_K(n_det, h, w)
    TCO = O.tco_init_from_boxes(boxes, K)
    rend = syn.make_renders(3, n_det, H, W)
    run = lambda: O.pose_predictor_forward(frames, K, obj, TCO, pts, None, lambda i, t, k: rend, 1, (H, W), backbone=tr.net_forward)
    run()
    t0 = time.time()
    for _ in range(calls):
        run()
    return t0, time.time(), n_det * calls


def cpu_all_cores(crop, budget_s=24.0):
    """The CPU port on ALL host cores, as the host's BEST (round 5's review: one 16-thread process at B = 1 beat sixteen 16-thread processes at
    B = 16 -- stock torch-CPU convolutions lose to thread placement on a 256-CPU host, so the figure understated the host).  The cores are filled
    with independent processes PINNED (sched_setaffinity) to disjoint runs of physical cores -- logical CPUs 0 .. n/2-1 when SMT doubles them --
    each running the loop on its own few detections; three shapes are tried (threads per process x detections per call: 4 x 1, 8 x 2, 16 x 4) and the best
    is reported with all of them beside it.  rate = detections processed by all processes / span from the first start to the last end."""
    import multiprocessing as mp
    ncpu = os.cpu_count() or 1
    try:
        avail = sorted(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        avail = list(range(ncpu))
    phys = avail[:max(1, len(avail) // 2)] if len(avail) >= 32 else avail      # SMT siblings are the upper half of the ids on the GPU boxes' EPYC hosts
    ctx = mp.get_context('spawn')
    tried = []
    for threads, n_det, calls in ((4, 1, 6), (8, 2, 4), (16, 4, 3)):
        procs = max(1, min(len(phys) // threads, 64))
        if procs * threads > len(phys) and tried:
            continue
        jobs = [(crop[0], crop[1], min(threads, len(phys)), calls, i, n_det, phys[i * threads:(i + 1) * threads] or None) for i in range(procs)]
        t_start = time.time()
        with ctx.Pool(procs) as pool:
            res = pool.map(_cpu_worker, jobs)
        t0, t1, n = min(r[0] for r in res), max(r[1] for r in res), sum(r[2] for r in res)
        tried.append(dict(value=round(n / (t1 - t0), 2), processes=procs, threads_per_process=min(threads, len(phys)), detections_per_call=n_det,
                          cores=procs * min(threads, len(phys)), pinned=True))
        budget_s -= time.time() - t_start
        if budget_s < 6.0:
            break
    best = max(tried, key=lambda d: d['value'])
    return dict(best, tried=tried)


def cpu_baseline(crop, repeats=3):
    """The oracle (torch-CPU port of the reference arithmetic + C geometry/roi_align) on a bounded sample (~25 s): one
    iteration of the loop at B = 1, 16, 64 detections (64 = the reference's bsz_objects) for the benched crop size and the
    other one beside it, one warm-up then the median of `repeats` (bop_predictions.py:132-134 times the reference the same
    way), at N threads; at 1 thread (the reference pins OMP_NUM_THREADS=1, cosypose/__init__.py:1-4) for B = 16.
    `value` = the best rate at the benched crop size."""
    sys.path.insert(0, os.path.join(REPO, 'oracle'))
    import torch
    import cosy_oracle as O
    from cosypose_amd import synthetic as syn
    sd = syn.golden_state_dict(0)
    tr = O.TorchRef(sd)
    pts = syn.make_mesh_points(7, 21, 2500)[:, np.random.RandomState(0).choice(2500, 2000, replace=False)]
    # the stock torch-CPU convolutions stop scaling at ~16 threads on the GPU box's 256-core host
    # (measured: 1 thread 10.3, 16 threads 17.3, 64 threads 10.6, 128 threads 3.7 crops/s at B=16)
    many = min(os.cpu_count() or 1, 16)

    def rate(H, W, n_det, cores):
        h, w = (512, 512) if H == W else (480, 640)
        obj, im, boxes = syn.make_detections(1, n_det, 2, 21, h, w)
        frames = syn.make_frames(2, 2, h, w)[im]
        K = syn.make_K(n_det, h, w)
        TCO = O.tco_init_from_boxes(boxes, K)
        rend = syn.make_renders(3, n_det, H, W)
        run = lambda: O.pose_predictor_forward(frames, K, obj, TCO, pts, None, lambda i, t, k: rend, 1, (H, W), backbone=tr.net_forward)
        torch.set_num_threads(cores)
        O.set_threads(cores)
        run()  # warm-up
        ts = []
        for _ in range(repeats):
            t0 = time.time(); run(); ts.append(time.time() - t0)
        return round(n_det / float(np.median(ts)), 3)
    sizes = [tuple(crop)] + [c for c in ((256, 256), (240, 320)) if c != tuple(crop)]
    table = {}
    for (H, W) in sizes:
        key = f'{H}x{W}'
        table[key] = {f'B={b}': rate(H, W, b, many) for b in (1, 16, 64)}
        table[key]['B=16, 1 thread'] = rate(H, W, 16, 1)
    key = '%dx%d' % tuple(crop)
    model, ncpu = host_cpu()
    try:
        allc = cpu_all_cores(tuple(crop))
    except Exception as e:      # noqa: BLE001 -- a reported figure, never a reason to lose the line
        allc = dict(value=None, error=f'{type(e).__name__}: {e}')
    one = max(table[key][f'B={b}'] for b in (1, 16, 64))
    best_all = allc.get('value') or 0.0
    # `value` = the host's best: the pinned all-cores run when it beats one process (then `cores` = the cores it used), else one `many`-thread process
    return dict(value=max(one, best_all), unit='pose-iterations/s', cores=allc.get('cores', many) if best_all > one else many, kind='port', all_cores=allc,
                value_one_process=one,
                value_1_thread=table[key]['B=16, 1 thread'], table=table, host=f'{model} ({ncpu} logical CPUs)',
                sample=f'1 iteration of the loop at B = 1 / 16 / 64 detections, {key} crops (and the other crop size beside it), fp32, torch-CPU '
                       f'backbone + C geometry/roi_align oracle; warm-up then median of {repeats}, {many} threads (and 1 thread at B = 16); '
                       f'host rates on this pool vary by +-40 % between boxes')


def oracle_deviation(torch, tc, pd, predictor_cls, coarse, refiner, labels, renders, crop, dtypes, n_sub=32, seed=1):
    """Part of the cpu_baseline leg (rank 0, N = 1): the first `n_sub` detections of the benched workload (config 1's generator, the bench's own
    coarse / refiner models and pre-generated renders), coarse 1 + refiner 4, through the HIP path in every benched storage type AND through the CPU
    oracle (torch-CPU backbone + C geometry / roi_align, fp32) -- the refined poses after all five iterations, per parameter group.  This is the
    bench line's own oracle comparison (round 5's `pose_deviation` compared with the fp32 HIP path only)."""
    sys.path.insert(0, os.path.join(REPO, 'oracle'))
    import cosy_oracle as O
    from cosypose_amd import synthetic as syn
    H, W = crop
    h, w = (512, 512) if H == W else (480, 640)
    n_obj = len(labels)
    obj, im, boxes = syn.make_detections(seed + 10, 256, 16, n_obj, h, w)
    obj, im, boxes = obj[:n_sub], im[:n_sub], boxes[:n_sub]
    frames, K = syn.make_frames(seed, 16, h, w), syn.make_K(16, h, w)
    rend_np = [r[:n_sub].cpu().numpy() for r in renders]
    pts = syn.make_mesh_points(7, n_obj, 2500)[:, np.random.RandomState(0).choice(2500, 2000, replace=False)]
    nthr = min(os.cpu_count() or 1, 16)
    torch.set_num_threads(nthr); O.set_threads(nthr)
    t0 = time.time()
    TCO = O.tco_init_from_boxes(boxes, K[im])
    c = O.pose_predictor_forward(frames[im], K[im], obj, TCO, pts, None, lambda n, t, k: rend_np[0], 1, (H, W),
                                 backbone=O.TorchRef(syn.golden_state_dict(0)).net_forward)
    r = O.pose_predictor_forward(frames[im], K[im], obj, c['iteration=1']['TCO_output'], pts, None, lambda n, t, k: rend_np[(1 + n) % len(rend_np)], 4, (H, W),
                                 backbone=O.TorchRef(syn.golden_state_dict(1)).net_forward)
    want = r['iteration=4']['TCO_output']
    oracle_s = time.time() - t0
    det = tc.PandasTensorCollection(infos=pd.DataFrame(dict(label=labels[obj], batch_im_id=im, score=1.0)), bboxes=torch.from_numpy(boxes).cuda())
    fr, Kd = torch.from_numpy(frames).cuda(), torch.from_numpy(K).cuda()
    out = {}
    keep = coarse.compute_dtype
    for dt in dtypes:
        for m in (coarse, refiner):
            m.compute_dtype = dt
            m.renderer.i = 0
        pred = predictor_cls(coarse_model=coarse, refiner_model=refiner, bsz_objects=n_sub, n_streams=1)
        final, _ = pred.get_predictions(fr, Kd, detections=det, n_coarse_iterations=1, n_refiner_iterations=4)
        a = final.poses.double().cpu().numpy().reshape(-1, 4, 4); b = np.asarray(want, np.float64).reshape(-1, 4, 4)
        rot = float(np.abs(a[:, :3, :3] - b[:, :3, :3]).max())
        tn = np.maximum(np.abs(b[:, :3, 3]).max(axis=1), 1e-12)
        tr = float((np.abs(a[:, :3, 3] - b[:, :3, 3]).max(axis=1) / tn).max())
        out[dt] = dict(rotation_abs=float('%.3g' % rot), translation_rel=float('%.3g' % tr), conforms=bool(max(rot, tr) <= 1e-4))
    for m in (coarse, refiner):
        m.compute_dtype = keep
    return dict(per_dtype=out, bound=1e-4, candidates=n_sub, oracle_seconds=round(oracle_s, 1),
                vs=f'CPU oracle (fp32, torch-CPU backbone + C geometry / roi_align, {nthr} threads): refined poses after coarse 1 + refiner 4 of the first '
                   f'{n_sub} detections of this workload, worst candidate')


def make_scene(syn, torch, tc, pd, labels, seed, D, n_frames, h, w, n_obj, with_poses=False):
    """(frames, K, table) of one frame size on the device; table = detections, or given poses for the refiner-only config"""
    frames = torch.from_numpy(syn.make_frames(seed, n_frames, h, w)).cuda()
    K = torch.from_numpy(syn.make_K(n_frames, h, w)).cuda()
    obj, im, boxes = syn.make_detections(seed + 10, D, n_frames, n_obj, h, w)
    infos = pd.DataFrame(dict(label=labels[obj], batch_im_id=im, score=1.0))
    if with_poses:
        return frames, K, tc.PandasTensorCollection(infos=infos, poses=torch.from_numpy(syn.make_TCO(seed + 20, D)).cuda())
    return frames, K, tc.PandasTensorCollection(infos=infos, bboxes=torch.from_numpy(boxes).cuda())


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(dirname, poses, preds, limit=DUMP_LIMIT_BYTES):
    """--dump-outputs: what one step returned, as DIR/<name>.npy in float32 -- `poses` (the refined poses of all candidates) and, when the path
    returns them, every stage / iteration's collection field by field (`refiner/iteration=4` -> refiner_iteration4_<field>).  The given initial
    poses of config 2 (`external_coarse`) are an input and are not written.  Above `limit` bytes in all, every array keeps the same fraction of
    its rows, chosen by a fixed seed (sorted)."""
    arrays = {'poses': poses}
    for key, coll in (preds or {}).items():
        if key == 'external_coarse':
            continue
        stage, it = key.split('/')
        for field, t in coll.tensors.items():
            arrays[f"{stage}_{it.replace('=', '')}_{field}"] = t
    arrays = {k: v.detach().float().cpu().numpy() for k, v in arrays.items()}
    total = sum(a.nbytes for a in arrays.values())
    if total > limit:
        frac = limit / total
        for k, a in arrays.items():
            keep = int(len(a) * frac)
            arrays[k] = a[np.sort(np.random.RandomState(0).choice(len(a), keep, replace=False))]
    os.makedirs(dirname, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(dirname, k + '.npy'), np.ascontiguousarray(a, dtype=np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--config', type=int, default=1, choices=[1, 2, 3], help='BASELINE.json configs[i] (see the module docstring)')
    ap.add_argument('--split', default='skewed', choices=['skewed', 'balanced'], help='config 3: how candidates are shared out')
    ap.add_argument('--crop', default='256x256', help='HxW of the crops: 256x256 (metric) or 240x320 (reference native)')
    ap.add_argument('--dtype', default=None, choices=['bf16', 'fp16', 'fp32'], help='storage type of the backbone; default fp16 (see the module docstring)')
    ap.add_argument('--detections', type=int, default=None, help='override the number of candidates (per GPU for config 1, total otherwise)')
    ap.add_argument('--bsz-objects', type=int, default=None,
                    help='crops per forward: default 256 for config 1 (BASELINE configs[1] names batch=256), 512 for configs 2 and 3 '
                         '(their batches are 1024 / 2048 candidates; 512 per forward measured +9 %% over 256, profiles/r02_batch_sweep.txt)')
    ap.add_argument('--streams', type=int, default=None,
                    help='HIP streams the chunks of a stage run on concurrently (CoarseRefinePosePredictor n_streams; default 2); with N > 1 and no '
                         '--bsz-objects the candidates of a rank are cut into N equal chunks')
    ap.add_argument('--full', action='store_true',
                    help='also measure everything beside the headline (single-stream schedule, collective alone, per-kernel pass / roofline, '
                         'bf16 / fp32 repeats and pose deviations, CPU baseline and oracle comparison); off by default')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='after the timed steps, write what the last timed step returned as DIR/<name>.npy (float32, <= 64 MB)')
    ap.add_argument('--no-cpu-baseline', action='store_true', help='with --full: skip the CPU baseline and the oracle comparison')
    ap.add_argument('--no-other-dtypes', action='store_true', help='with --full: skip the bf16 / fp32 repeats of the timed loop and the deviation pass')
    ap.add_argument('--no-profile', action='store_true', help='with --full: skip the per-kernel HIP-event pass (no roofline object)')
    ap.add_argument('--layers', action='store_true', help='print the per-launch table to stderr (implies --full: the table comes from its per-kernel pass)')
    ap.add_argument('--renderer', default='pregenerated', choices=['pregenerated', 'hip'],
                    help="renderer.render source: pre-generated device images (default: the reference's renderer is outside the "
                         "path) or the on-device HIP rasteriser (SURVEY 8f-1) rendering every crop in every iteration")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error('--steps must be at least 1')
    if args.layers:
        args.full = True

    import torch
    import torch.distributed as dist
    import pandas as pd
    from cosypose_amd import synthetic as syn, _lib
    from cosypose_amd import tensor_collection as tc
    from cosypose_amd.mesh_db import BatchedMeshes
    from cosypose_amd.pose_predictor import CoarseRefinePosePredictor
    from cosypose_amd.distributed import (init_distributed_mode, all_gather_rows, local_device_index, get_predictions_sharded,
                                          get_predictions_sharded_scenes, plan_shards, self_launch, process_group_info)

    if not torch.cuda.is_available():
        raise SystemExit('bench.py needs an MI355X (no CPU fallback)')
    # `python bench.py --gpus N` (the driver's command shape) launches its own N ranks; under torch.distributed.run it is a rank
    rc = self_launch(args.gpus)
    if rc is not None:
        raise SystemExit(rc)
    rank, world = init_distributed_mode('nccl')
    if world != args.gpus:
        raise SystemExit(f'--gpus {args.gpus} but WORLD_SIZE={world}: the launcher and the flag disagree')
    torch.cuda.set_device(local_device_index())
    H, W = (int(v) for v in args.crop.split('x'))
    cfg_i = args.config
    dtype = args.dtype or 'fp16'
    n_obj = 30 if cfg_i == 2 else 21
    n_coarse, n_refine = (0, 4) if cfg_i == 2 else (1, 4)
    labels = np.array([f'obj_{i:06d}' for i in range(1, n_obj + 1)])
    pts = syn.make_mesh_points(7, n_obj, 2500)
    infos = {l: dict(label=l, n_points=2500, n_sym=1) for l in labels}
    mesh_db = BatchedMeshes(infos, labels, torch.from_numpy(pts), torch.eye(4).reshape(1, 1, 4, 4).repeat(n_obj, 1, 1, 1)).float().cuda()

    # ---- workload
    if cfg_i == 1:
        D = args.detections or 256
        h, w = (512, 512) if H == W else (480, 640)   # square frames for square crops
        scenes = [make_scene(syn, torch, tc, pd, labels, 1 + rank, D, 16, h, w, n_obj)]      # each rank its own candidates (weak scaling)
        total, scaling, per_rank = D * world, 'weak', [D] * world
        desc = f'BASELINE configs[1]: {D} detections/GPU over 16 frames {h}x{w}, {n_obj} objects'
    elif cfg_i == 2:
        D = args.detections or 1024
        scenes = [make_scene(syn, torch, tc, pd, labels, 2, D, 64, 540, 720, n_obj, with_poses=True)]
        total, scaling = D, 'strong'
        per_rank = [len(p) for p in plan_shards(D, world)]
        desc = f'BASELINE configs[2]: {D} candidates over 64 frames 540x720, {n_obj} objects (T-LESS shape), refiner-only from given poses'
    else:
        D = args.detections or 2048
        sizes = [(480, 640)] * 5 + [(540, 720), (960, 1280)]
        share = [D // 7 + (1 if g < D % 7 else 0) for g in range(7)]
        scenes = [make_scene(syn, torch, tc, pd, labels, 30 + g, share[g], 8, hh, ww, n_obj) for g, (hh, ww) in enumerate(sizes)]
        total, scaling = D, 'strong'
        if args.split == 'skewed':
            frac = np.array(SKEW[:world] if world <= 8 else SKEW + [64] * (world - 8), dtype=np.float64)
            cnt = np.floor(frac / frac.sum() * D).astype(int); cnt[0] += D - cnt.sum()
            plan_kw = dict(balance='counts', counts=cnt.tolist())
        else:
            plan_kw = dict(balance='cost')
        per_rank = [len(p) for p in plan_shards(D, world, **plan_kw)]
        desc = (f'BASELINE configs[3]: {D} candidates over 7 datasets (5x 640x480, 720x540, 1280x960 frames), {n_obj} objects, '
                f'{args.split} shares {per_rank}')
    full_bsz = 256 if cfg_i == 1 else 512          # crops per forward of the single-stream schedule (and of the per-kernel event pass)
    if args.streams is None:
        args.streams = DEFAULT_STREAMS
    if args.bsz_objects is None:
        args.bsz_objects = full_bsz if args.streams <= 1 else max(16, -(-min(max(per_rank), full_bsz) // args.streams))
    cap = min(max(per_rank), max(args.bsz_objects, full_bsz))
    g = torch.Generator(device='cuda'); g.manual_seed(1 + rank)
    renders = [torch.rand(cap, 3, H, W, device='cuda', generator=g) for _ in range(5)]
    renderer = SyntheticRenderer(renders)
    if args.renderer == 'hip':
        from cosypose_amd.rasterizer import RenderMeshes, HipBatchRenderer
        mv, mf, mc = syn.make_render_meshes(7, n_obj, n_lat=48, n_lon=64)        # 6,016 triangles per object
        renderer = HipBatchRenderer(RenderMeshes(labels, mv, mf, mc).cuda())
    coarse = build_model(0, mesh_db, (H, W), dtype, renderer)
    refiner = build_model(1, mesh_db, (H, W), dtype, renderer)
    predictor = CoarseRefinePosePredictor(coarse_model=coarse, refiner_model=refiner, bsz_objects=args.bsz_objects, n_streams=args.streams)
    if args.streams > 1 and not predictor._streams_usable():      # a renderer that declines concurrent streams: the chunks would run one after the other -> one full-size launch instead
        args.streams, args.bsz_objects = 1, min(max(per_rank), full_bsz)
        predictor.n_streams, predictor.bsz_objects = 1, args.bsz_objects
    iters_total = total * (n_coarse + n_refine)
    gather_us = []
    use_dist = dist.is_available() and dist.is_initialized()     # world > 1, or a forced 1-rank RCCL group (COSY_FORCE_DIST=1)
    last_outputs = {}       # --dump-outputs: the per-iteration collections the last step returned

    def step(local_only=False):
        preds = None
        if cfg_i == 1:
            frames, K, det = scenes[0]
            final, preds = predictor.get_predictions(frames, K, detections=det, n_coarse_iterations=n_coarse, n_refiner_iterations=n_refine)
            poses = final.poses
            if use_dist and not local_only:
                poses = all_gather_rows(poses, counts=per_rank)   # ONE collective: refined poses of all ranks, rank order
        elif cfg_i == 2:
            frames, K, init = scenes[0]
            final, preds = get_predictions_sharded(predictor, frames, K, data_TCO_init=init, n_coarse_iterations=0, n_refiner_iterations=n_refine)
            poses = final.poses
        else:
            poses, _ = get_predictions_sharded_scenes(predictor, scenes, n_coarse, n_refine, **plan_kw)
        if args.dump_outputs:
            last_outputs['preds'] = preds
        return poses

    def sync():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # Python's cyclic collector: a full (generation 2) pass over the process's ~10^6 long-lived objects (torch, pandas) takes
    # ~60 ms of host time on this box (profiles/exp/gcprobe.py) -- 2.5 steps of GPU work, and the host only leads the GPU by
    # a few steps.  The long-lived objects are moved to the permanent generation, so passes during the steps only look at what
    # the steps allocate.  Done behind the FIRST warm-up step (which builds the engines, plans and caches that are to be frozen), not
    # between the warm-up and the timed steps: 60 ms with nothing queued let the GPU's clocks fall back to idle right in front of
    # the timed region (COSY_BENCH_GC_LATE=1: the old order, for the A/B in profiles/r04_dead_ends.txt / DESIGN section 5).
    gc_late = os.environ.get('COSY_BENCH_GC_LATE') == '1'
    out = step()                # the first warm-up step (--warmup 0: the checks and the engines' first-call set-up still happen once, untimed)
    if not gc_late:
        gc.collect()
        gc.freeze()
    for _ in range(args.warmup - 1):
        out = step()
    assert torch.isfinite(out).all(), 'non-finite refined poses'
    assert out.shape == (total, 4, 4)
    profile = args.full and not args.no_profile
    gather_us.clear()
    if gc_late:
        gc.collect()
        gc.freeze()
    if os.environ.get('COSY_BENCH_NOSYNC') != '1':      # diagnostic only (step_ms of a run that never drained the queues): the line is not a measurement then
        sync()
    t0 = time.perf_counter()
    host_ms = []
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]     # one event per step boundary on the caller's stream (no synchronisation)
    marks[0].record()
    for i in range(args.steps):
        th = time.perf_counter()
        last_poses = step()
        marks[i + 1].record()
        host_ms.append((time.perf_counter() - th) * 1e3)   # host enqueue time of the step (the GPU runs behind)
    sync()
    dt = time.perf_counter() - t0
    step_ms = [marks[i].elapsed_time(marks[i + 1]) for i in range(args.steps)]
    if args.layers and rank == 0:
        print('host enqueue ms/step: ' + ' '.join(f'{v:.2f}' for v in host_ms), file=sys.stderr)
    if world > 1:
        t = torch.tensor([dt], device='cuda', dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, last_poses, last_outputs.get('preds'))
    last_outputs.clear()
    # the same K steps as ONE stream of full-size launches (the schedule of rounds 1-3's lines), reported beside the headline
    single = None
    if args.full and args.streams > 1 and not args.no_other_dtypes:
        predictor.n_streams, predictor.bsz_objects = 1, min(max(per_rank), full_bsz)
        step()
        k1 = max(2, min(args.steps, 8))
        sync(); t1 = time.perf_counter()
        for _ in range(k1):
            step()
        sync(); d1 = time.perf_counter() - t1
        if world > 1:
            tt = torch.tensor([d1], device='cuda', dtype=torch.float64); dist.all_reduce(tt, op=dist.ReduceOp.MAX); d1 = float(tt.item())
        single = dict(value=round(iters_total * k1 / d1, 1), ms_per_step=round(1e3 * d1 / k1, 3), steps=k1, bsz_objects=predictor.bsz_objects, streams=1)
        predictor.n_streams, predictor.bsz_objects = args.streams, args.bsz_objects
    # the collective alone, timed in its own pass (device events around the call; nothing is drained inside the timed region)
    if args.full and use_dist and cfg_i == 1:
        local = step(local_only=True)
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); all_gather_rows(local, counts=per_rank); e1.record(); e1.synchronize()
            gather_us.append(e0.elapsed_time(e1) * 1e3)
    # Per-kernel timing for `roofline`: the SAME steps again with a HIP event recorded on the launch stream after every
    # backbone launch.  Kept out of the timed region on purpose: one event per kernel serialises back-to-back
    # launches and costs ~6 % of the headline value (measured 34.4k vs 32.3k pose-iter/s).
    # With --streams > 1 this pass runs the single-stream schedule (one launch of `full_bsz` crops per kernel): under
    # concurrency a kernel's start-to-end time includes the other chunks' kernels sharing the chip and is not a kernel property.
    prof_steps = min(args.steps, 4)
    prof_bsz = min(max(per_rank), full_bsz)
    if profile:
        predictor.n_streams, predictor.bsz_objects = 1, prof_bsz
        nets = [m._net(prof_bsz, out.device) for m in ([refiner] if cfg_i == 2 else [coarse, refiner])]
        for n_ in nets:
            _lib.check(_lib.lib().cosy_effnet_b3_set_profiling(n_, 1))
        for _ in range(prof_steps):
            step()
        sync()
        predictor.n_streams, predictor.bsz_objects = args.streams, args.bsz_objects

    roofline = None
    if profile and rank == 0:
        recs = []
        for n_ in nets:
            recs += _lib.profile_read(n_)
            _lib.check(_lib.lib().cosy_effnet_b3_set_profiling(n_, 0))

        def agg(key):
            out = {}
            for r in recs:
                k = out.setdefault(key(r), dict(ms=0.0, bytes=0.0, flops=0.0, cbytes=0.0, n=0, layers=set()))
                k['ms'] += r['ms_avg'] * r['n']; k['bytes'] += r['bytes'] * r['n']; k['flops'] += r['flops'] * r['n']; k['n'] += r['n']
                k['cbytes'] += r['cbytes'] * r['n']; k['layers'].add(r['layer'])
            return out
        import ctypes
        front_kind = {}
        for i_ in range(26):
            dims_ = (ctypes.c_int * 11)()
            _lib.check(_lib.lib().cosy_effnet_b3_block_info(nets[0], i_, dims_))
            front_kind[i_] = int(dims_[7])
        kinds = agg(lambda r: r['name'])
        fams = agg(lambda r: r['name'].split('<')[0].split('+')[0])
        total_ms = sum(k['ms'] for k in kinds.values())
        n_fw = sum(r['n'] for r in recs if r['name'].startswith('stem_'))      # forwards timed
        if args.layers:
            per = agg(lambda r: (r['layer'], r['name']))
            for (layer, name), k in per.items():
                print(f"{layer:3d} {name:34s} n={k['n']:4d} {k['ms'] / max(n_fw, 1) * 1e3:9.1f} us/fwd  {k['bytes'] / k['ms'] / 1e6:8.1f} GB/s "
                      f"{k['flops'] / k['ms'] / 1e9:8.1f} TFLOP/s", file=sys.stderr)
            for table in (fams, kinds):
                for name, k in sorted(table.items(), key=lambda kv: -kv[1]['ms']):
                    print(f"{name:34s} {100 * k['ms'] / total_ms:5.1f}%  avg {k['ms'] / k['n'] * 1e3:8.1f} us  {k['bytes'] / k['ms'] / 1e6:8.1f} GB/s "
                          f"{k['flops'] / k['ms'] / 1e9:8.1f} TFLOP/s", file=sys.stderr)

        def line(name, k):
            intensity = k['flops'] / k['bytes']
            balance = MFMA_PEAK_TFLOPS[dtype] * 1e12 / (HBM_PEAK_GBS * 1e9)
            if intensity < balance:
                ach = k['bytes'] / k['ms'] / 1e6
                d = dict(bound='hbm', achieved=round(ach, 1), peak=HBM_PEAK_GBS, unit='GB/s', frac=round(ach / HBM_PEAK_GBS, 4))
            else:
                ach = k['flops'] / k['ms'] / 1e9
                d = dict(bound='mfma', achieved=round(ach, 1), peak=MFMA_PEAK_TFLOPS[dtype], unit='TFLOP/s', frac=round(ach / MFMA_PEAK_TFLOPS[dtype], 4))
            d.update(kernel=name, launches_timed=k['n'], avg_launch_us=round(k['ms'] / k['n'] * 1e3, 2),
                     algorithmic_bytes_per_launch=round(k['bytes'] / k['n']), algorithmic_flops_per_launch=round(k['flops'] / k['n']),
                     share_of_backbone_time=round(k['ms'] / total_ms, 4))
            # the same launch priced by its COMPULSORY bytes only (SURVEY 8(d)'s block-fused model: block inputs / outputs / residuals and
            # weights; the depthwise output D and the other block-internal tensors count as 0) -- what `frac` would be if D never left the chip
            d['compulsory_bytes_per_launch'] = round(k['cbytes'] / k['n'])
            d['compulsory_frac'] = round(k['cbytes'] / k['ms'] / 1e6 / HBM_PEAK_GBS, 4)
            vb = valu_bound(name, k, prof_bsz, (H, W), front_kind)
            if vb:
                d['valu_bound'] = vb
            return d
        fam_name, fam = max(fams.items(), key=lambda kv: kv[1]['ms'])
        members = {n: k for n, k in kinds.items() if n.split('<')[0].split('+')[0] == fam_name}
        inst_name, inst = max(members.items(), key=lambda kv: kv[1]['ms'])
        roofline = line(inst_name, inst)                       # the dominant instantiation of the dominant family
        roofline['family'] = line(fam_name, fam)               # ... and the whole family (every instantiation together)
        # the family's next instantiations by time (blocks 3 / 4 and blocks 14-17 of the wave front are within 1 % of each other: which of
        # them leads changes from build to build, so both are always in the line)
        roofline['next_instantiations'] = [line(n_, k_) for n_, k_ in sorted(members.items(), key=lambda kv: -kv[1]['ms']) if n_ != inst_name][:2]
        roofline['traffic'] = None
        # HBM bytes per launch from PMC counters cannot be measured from inside this process (rocprofv3 = separate process): taken from the
        # newest profiles/r*_pmc_traffic.json that was collected for exactly these kernel sources and this dtype, else null.  rocprofv3 names an
        # instantiation with ALL its template arguments, this table with the leading ones: match by prefix, launches-weighted over the matches.
        import glob
        note = 'HBM counters need rocprofv3 (separate process): see profiles/collect_all.sh'
        tj_use = None
        if cfg_i == 1 and args.crop == '256x256' and (args.detections or 256) == 256:
            for tfile in sorted(glob.glob(os.path.join(REPO, 'profiles', 'r*_pmc_traffic.json')), reverse=True):
                tj = json.load(open(tfile))
                if tj.get('csrc_sha') == csrc_sha() and tj.get('dtype', 'bf16') == dtype:
                    tj_use = tj
                    note = f"profiles/{os.path.basename(tfile)} (PMC passes of this command on kernel sources {tj['csrc_sha']})"
                    break
            else:
                note = 'no profiles/r*_pmc_traffic.json was collected for these kernel sources: not reported'

        def traffic_for(name):
            if not tj_use or '<' not in name:
                return None
            stem = name[:-1]
            hits = [v for k_, v in tj_use.get('kernels', {}).items() if k_ == name or k_.startswith(stem + ',')]
            nl = sum(v['launches'] for v in hits)
            return round(sum((v['read_bytes'] + v['write_bytes']) * v['launches'] for v in hits) / nl) if nl else None
        roofline['traffic'] = traffic_for(inst_name)
        for n_ in roofline['next_instantiations']:
            n_['traffic'] = traffic_for(n_['kernel'])
        # the other kernel families by time, each with its leading instantiation: the line always shows the fused MBConv fronts (mbconv_wave_kernel: the
        # dominant family until round 5, 0.175 of the HBM roof on blocks 14-17 then) beside the 1x1-conv GEMMs, whichever of the two leads the build
        others = []
        for fn_, fk_ in sorted(fams.items(), key=lambda kv: -kv[1]['ms']):
            if fn_ == fam_name or len(others) >= 2:
                continue
            mem_ = {n: k for n, k in kinds.items() if n.split('<')[0].split('+')[0] == fn_}
            top_ = sorted(mem_.items(), key=lambda kv: -kv[1]['ms'])[:3]
            insts_ = []
            for n__, k__ in top_:
                l__ = line(n__, k__)
                l__['traffic'] = traffic_for(n__)
                insts_.append(l__)
            others.append(dict(family=line(fn_, fk_), instantiations=insts_))
        roofline['other_families'] = others
        roofline['traffic_source'] = note
        roofline['backbone_ms_per_forward'] = round(total_ms / max(n_fw, 1), 3)
        roofline['launch'] = (f'{prof_bsz} crops per launch, timed with one HIP event per launch in a single-stream pass after the timed region' +
                              (f'; the timed region runs the same kernels as {args.streams} concurrent streams of {args.bsz_objects}-crop launches'
                               if args.streams > 1 else ''))

    # ---- the same timed loop in the other storage types, and the benched type's pose deviation from the fp32 HIP path
    other, deviation = {}, None
    if args.full and not args.no_other_dtypes and args.renderer == 'pregenerated':
        def run_first(models):
            for m in models:
                m.renderer.i = 0          # same synthetic renders for every dtype
            return step(local_only=True).clone()
        ref_models = None
        got_main = run_first([coarse, refiner])
        for od in [d for d in ('bf16', 'fp16', 'fp32') if d != dtype]:
            for m in (coarse, refiner):
                m.compute_dtype = od
            got = run_first([coarse, refiner])
            if od == 'fp32':
                ref_models = got
            for _ in range(max(1, min(args.warmup, 1))):
                step()
            k_steps = max(2, min(args.steps, 6))
            sync(); t1 = time.perf_counter()
            for _ in range(k_steps):
                step()
            sync(); d1 = time.perf_counter() - t1
            if world > 1:
                tt = torch.tensor([d1], device='cuda', dtype=torch.float64); dist.all_reduce(tt, op=dist.ReduceOp.MAX); d1 = float(tt.item())
            other[od] = dict(value=round(iters_total * k_steps / d1, 1), ms_per_step=round(1e3 * d1 / k_steps, 3), steps=k_steps, poses=got)
        for m in (coarse, refiner):
            m.compute_dtype = dtype

        def dev_of(a, b):
            a = a.double().cpu().numpy().reshape(-1, 4, 4); b = b.double().cpu().numpy().reshape(-1, 4, 4)
            rot = float(np.abs(a[:, :3, :3] - b[:, :3, :3]).max())
            tn = np.maximum(np.abs(b[:, :3, 3]).max(axis=1), 1e-12)
            return dict(rotation_abs=float('%.3g' % rot), translation_rel=float('%.3g' % (np.abs(a[:, :3, 3] - b[:, :3, 3]).max(axis=1) / tn).max()))
        ref = ref_models if dtype != 'fp32' else got_main
        if ref is not None:
            if dtype != 'fp32':
                deviation = dict(dev_of(got_main, ref), vs='fp32 HIP path, same workload, refined poses after all iterations, worst of '
                                 f'{got_main.shape[0]} candidates', bound=1e-4)
                deviation['conforms'] = bool(max(deviation['rotation_abs'], deviation['translation_rel']) <= 1e-4)
            for od, v in other.items():
                p_ = v.pop('poses')
                if od != 'fp32':
                    v['pose_deviation'] = dev_of(p_, ref)
                    v['conforms'] = bool(max(v['pose_deviation'].values()) <= 1e-4)     # north_star: <= 1e-4 on pose parameters
        for v in other.values():
            v.pop('poses', None)

    if rank == 0:
        value = iters_total * args.steps / dt
        mb = ALGO_MB_PER_POSE_ITER.get((dtype, H))
        line_ = {
            'metric': 'refined pose-iterations/sec (256x256 crops, n_iter=1+4)' if (H == W and cfg_i != 2) else
                      f'refined pose-iterations/sec ({H}x{W} crops, n_iter={n_coarse}+{n_refine})',
            'value': round(value, 1), 'unit': 'pose-iterations/s', 'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup,
            'ms_per_step': round(1e3 * dt / args.steps, 3), 'higher_is_better': True, 'scaling': scaling, 'vs_baseline': None,
            'dtype': dtype, 'data': 'synthetic',
            'dtype_note': 'BASELINE configs[1] names bf16; bf16 storage misses north_star\'s 1e-4 pose bound, fp16 (same bytes, same MFMA '
                          'rate) meets it: the headline is fp16, bf16 / fp32 are timed beside it in other_dtypes (--full)',
            'config_deviation': ({'field': 'dtype', 'baseline': NAMED_DTYPE[cfg_i], 'benched': dtype,
                                  'reason': 'the named type misses north_star\'s 1e-4 pose bound (see other_dtypes.%s: conforms false); same bytes, same '
                                            'MFMA rate; do not compare `value` with a number quoted on the named type without reading other_dtypes' % NAMED_DTYPE[cfg_i]}
                                 if NAMED_DTYPE[cfg_i] != dtype else None),
            'pose_deviation': deviation, 'other_dtypes': other or None,
            'config': {'workload': desc + f', coarse {n_coarse} + refiner {n_refine} iterations, {H}x{W} crops, ' +
                                   ('synthetic on-device renders' if args.renderer == 'pregenerated' else
                                    'renders by the on-device HIP rasteriser (6k-triangle meshes) inside the loop'),
                       'pose_iterations_per_step': iters_total, 'candidates_per_rank': per_rank, 'bsz_objects': args.bsz_objects,
                       'streams': args.streams,
                       'parallelism': f'candidate-sharded x{world}, 1 all-gather of refined poses per step' + (' (RCCL, forced 1-rank group)' if use_dist and world == 1 else ''),
                       'single_stream': single,
                       'step_ms': {'each': [round(v, 2) for v in step_ms], 'note': 'device time between step boundaries on the caller\'s stream (events, rank 0); the first follows a synchronisation: empty queues'},
                       'all_gather_us': round(float(np.median(gather_us)), 1) if gather_us else None,
                       'process_group': process_group_info()},
            'roofline': roofline,
            'path_hbm_frac': round(value / world * mb * 1e6 / (HBM_PEAK_GBS * 1e9), 5) if mb else None,
            'cpu_baseline': None,
        }
        if args.full and world == 1 and not args.no_cpu_baseline:
            if cfg_i == 1 and args.renderer == 'pregenerated':
                try:      # the bench line's own comparison with the ORACLE (32-crop subset, all five iterations), every benched storage type
                    vo = oracle_deviation(torch, tc, pd, CoarseRefinePosePredictor, coarse, refiner, labels, renders, (H, W),
                                          [dtype] + ([d for d in ('bf16', 'fp16', 'fp32') if d != dtype] if not args.no_other_dtypes else []))
                    if line_['pose_deviation'] is None:
                        line_['pose_deviation'] = {}
                    line_['pose_deviation']['vs_oracle'] = dict(vo, **vo['per_dtype'][dtype])
                    for od, v in (line_['other_dtypes'] or {}).items():
                        if od in vo['per_dtype']:
                            v['pose_deviation_vs_oracle'] = vo['per_dtype'][od]
                            v['conforms'] = bool(v.get('conforms', True) and vo['per_dtype'][od]['conforms']) if od != 'fp32' else vo['per_dtype'][od]['conforms']
                except Exception as e:      # noqa: BLE001 -- reported beside the line, never a reason to lose it
                    line_.setdefault('notes', []).append(f'oracle deviation leg failed: {type(e).__name__}: {e}')
            line_['cpu_baseline'] = cpu_baseline((H, W))
        print(json.dumps(line_), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
