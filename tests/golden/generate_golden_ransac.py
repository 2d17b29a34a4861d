#!/usr/bin/env python3
"""Generate tests/golden/reference_golden_ransac.npz: the REFERENCE's own multi-view candidate matching
(cosypose/multiview/ransac.py with its compiled cosypose_cext, run in place, FLOAT32 on the CPU, one thread) on seeded synthetic scenes
(cosypose_amd.synthetic.make_ba_scene with 8 bounding-box corners per mesh and the true obj_id withheld).
Run in the build container only:   python tests/golden/generate_golden_ransac.py

Shims as in generate_golden_ba.py: generate_golden.install_stubs, np.int = int, cosypose_cext from oracle/_ref, one thread.  The
fixture holds arrays and id / label columns only.

  STAGE fixtures (prefix a_: seed 162, 6 objects, 4 views, n_ransac_iter 2000; b_: seed 164, 12 objects, 8 views, 50): the reference's
  seeds, the tentative matches per view pair, per seed its TC1C2, the chosen symmetry, the runner-up gap and the distance of every
  symmetry of match 1's label; the distance of every (hypothesis, tentative match); per hypothesis n_inliers / dists_sum (recomputed
  here from the reference's distances and ASSERTED to reproduce find_ransac_inliers' output) and whether it is left out of the
  n_inliers comparison (a distance within 1e-4 of the threshold, or two conflicting inliers within 1e-4 of each other); the
  reference's best hypotheses and inlier matches.
  END-TO-END fixtures (a_, c_: scene 164 at 2000, d_: seed 3, 10 objects, 5 views): seeds, filtered candidates, partition, view pairs,
  scene_infos, the winners' n_inliers and, per view pair, the largest rotation / translation error against the scene's true
  relative camera pose among the reference's hypotheses that reach the winner's n_inliers.  A scene is admitted only if the
  reference in float32 and in float64 agree on everything the end-to-end test compares.
  k_: scene 162 with known camera poses.  e_: seed 161 (3 objects, 3 views), where the reference returns nothing.

The generator asserts what the tests rely on; if a seed violates a condition, change the seed, not the bound.
"""
import sys
import pathlib

HERE = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import numpy as np
import torch

import generate_golden as gg
from generate_golden_ba import save_npz
from cosypose_amd import synthetic as syn

THRESHOLD = 0.02
N_MIN_INLIERS = 3
NEAR = 1e-4
SCENE_KEYS = ('pts', 'sym', 'n_sym', 'cand_view_id', 'cand_obj_id', 'cand_label_id', 'cand_score', 'cand_poses', 'cam_view_id', 'cam_K', 'cam_TWC')
SEED_KEYS = ('view1', 'view2', 'match1_cand1', 'match1_cand2', 'match2_cand1', 'match2_cand2')


def reference():
    gg.install_stubs()
    sys.path.insert(0, str(gg.REPO / 'oracle' / '_ref'))
    np.int = int
    torch.set_num_threads(1)
    import cosypose_cext
    from cosypose.lib3d.rigid_mesh_database import BatchedMeshes
    from cosypose.lib3d import symmetric_distances as sdist
    from cosypose.lib3d.transform_ops import invert_T
    from cosypose.multiview import ransac
    import cosypose.utils.tensor_collection as tc
    return dict(cext=cosypose_cext, BatchedMeshes=BatchedMeshes, sdist=sdist, invert_T=invert_T, ransac=ransac, tc=tc)


def collections(R, scene, dtype):
    cand, cams, _, mesh_db = syn.ba_scene_collections(dict(scene, pair_view1=np.zeros(0, np.int64), pair_view2=np.zeros(0, np.int64),
                                                           pair_TC1C2=np.zeros((0, 4, 4))), R['BatchedMeshes'], dtype=dtype,
                                                      collection=R['tc'].PandasTensorCollection)
    cand.infos = cand.infos.drop(columns=['obj_id'])
    cand.infos['cand_id'] = np.arange(len(cand))
    cams.register_tensor('TWC', torch.as_tensor(scene['cam_TWC']).to(dtype))
    return cand, cams, mesh_db


def hypotheses_detail(R, cand, seeds, mesh_db, TC1C2_ref):
    """What decided each of the reference's hypotheses: its distance function evaluated here once per symmetry index k of match 1's
    label, for all seeds at once -> (H,S) distances (inf beyond the label's n_sym), the first minimum of each row (the tie rule of
    scatter_argmin), asserted to give the reference's TC1C2 bit for bit."""
    label = cand.infos['label'].values
    m1a, m1b, m2a, m2b = (np.asarray(seeds[k]) for k in SEED_KEYS[2:])
    mesh_row = np.array([mesh_db.label_to_id[l] for l in label[m1a]])
    n_sym = np.array([mesh_db.n_sym_mapping[l] for l in label[m1a]])
    T_a, T_b_inv, T_g, T_d = cand.poses[m1a], R['invert_T'](cand.poses[m1b]), cand.poses[m2a], cand.poses[m2b]
    S = mesh_db.symmetries.shape[1]
    table = np.full((len(m1a), S), np.inf, np.float32)
    for k in range(S):
        d, _ = R['sdist'].symmetric_distance_batched_fast(T_g, T_a @ mesh_db.symmetries[mesh_row, k] @ T_b_inv @ T_d, label[m2a], mesh_db)
        table[:, k] = np.where(k < n_sym, d.numpy(), np.inf)
    chosen = table.argmin(1)
    assert torch.equal(T_a @ mesh_db.symmetries[mesh_row, chosen] @ T_b_inv, TC1C2_ref), 'the rows do not explain the reference\'s choice'
    return chosen.astype(np.int32), table


def compact_tmatches(seeds, tm):
    """per ordered view pair the tentative matches of its first hypothesis; asserted equal for every other hypothesis of the pair"""
    hyp, c1, c2 = (np.asarray(tm[k]) for k in ('hypothesis_id', 'cand1', 'cand2'))
    H = len(seeds['view1'])
    counts = np.bincount(hyp, minlength=H)
    starts = np.concatenate([[0], np.cumsum(counts)])
    pv1, pv2, off, o1, o2, hyp_pair, lists = [], [], [0], [], [], np.zeros(H, np.int32), {}
    for h in range(H):
        key = (int(seeds['view1'][h]), int(seeds['view2'][h]))
        l = (c1[starts[h]:starts[h + 1]], c2[starts[h]:starts[h + 1]])
        if key not in lists:
            assert not pv1 or key > (pv1[-1], pv2[-1]), 'view pairs not ascending'
            lists[key] = (len(pv1), l)
            pv1.append(key[0]); pv2.append(key[1]); o1.append(l[0]); o2.append(l[1]); off.append(off[-1] + len(l[0]))
        else:
            assert np.array_equal(lists[key][1][0], l[0]) and np.array_equal(lists[key][1][1], l[1])
        hyp_pair[h] = lists[key][0]
    return dict(pair_view1=np.array(pv1, np.int32), pair_view2=np.array(pv2, np.int32), pair_off=np.array(off, np.int64),
                pair_cand1=np.concatenate(o1).astype(np.int32), pair_cand2=np.concatenate(o2).astype(np.int32), hyp_pair=hyp_pair), starts


def walk(c1, c2, d):
    """one hypothesis: inliers ordered by (distance, position), each cand1 / cand2 once -> (n_inliers, float32 sum, matches, near-tie flag)"""
    pos = np.flatnonzero(d <= np.float32(THRESHOLD))
    pos = pos[np.argsort(d[pos], kind='stable')]
    used1, used2, total, matches, conflict = set(), set(), np.float32(0), [], False
    for n, i in enumerate(pos):
        for j in pos[:n]:                   # a conflicting inlier (shared candidate) whose distance is within NEAR: the order may flip
            if (c1[i] == c1[j] or c2[i] == c2[j]) and abs(float(d[i]) - float(d[j])) < NEAR:
                conflict = True
        if c1[i] in used1 or c2[i] in used2:
            continue
        used1.add(c1[i]); used2.add(c2[i])
        total = np.float32(total + d[i])
        matches.append((int(c1[i]), int(c2[i])))
    return len(matches), total, matches, conflict


def run(R, scene, n_iter, dtype, cameras=False):
    """the reference's pipeline step by step (ransac.py:137-199), every intermediate kept"""
    rs = R['ransac']
    cand, cams, mesh_db = collections(R, scene, dtype)
    mesh_db = mesh_db.to(dtype)
    seeds, tm = R['cext'].make_ransac_infos(cand.infos['view_id'].values.tolist(), cand.infos['label'].values.tolist(), 1 if cameras else n_iter, 0)
    out = dict(seeds=seeds, tm=tm, cand=cand)
    if len(seeds['view1']) == 0:
        return out
    with torch.no_grad():
        if cameras:
            idx = {v: n for n, v in enumerate(cams.infos['view_id'])}
            TC1C2 = R['invert_T'](cams.TWC[[idx[v] for v in seeds['view1']]]) @ cams.TWC[[idx[v] for v in seeds['view2']]]
        else:
            TC1C2 = rs.estimate_camera_poses_batch(cand, seeds, mesh_db, bsz=10 ** 9)
            if dtype == torch.float32:
                out['sym'], out['sym_dists'] = hypotheses_detail(R, cand, seeds, mesh_db, TC1C2)
        dists = rs.score_tmaches_batch(cand, tm, TC1C2, mesh_db, bsz=10 ** 9)
    inl = R['cext'].find_ransac_inliers(seeds['view1'], seeds['view2'], tm['hypothesis_id'], tm['cand1'], tm['cand2'],
                                        dists.float().numpy(), THRESHOLD, N_MIN_INLIERS)
    out.update(TC1C2=TC1C2.numpy(), dists=dists.float().numpy(), inliers=inl)
    out['pairs'] = rs.get_best_viewpair_pose_est(TC1C2, seeds, inl)
    out['filtered'] = rs.scene_level_matching(cand, inl)
    out['scene_infos'] = rs.make_obj_infos(out['filtered']) if len(out['filtered']) else None
    return out


def partition(ids):
    groups = {}
    for n, i in enumerate(ids):
        groups.setdefault(int(i), []).append(n)
    return sorted(tuple(g) for g in groups.values())


def pose_errors(T, truth):
    """rotation angle (rad) and translation error (m) of T against truth"""
    dR = T[:3, :3].astype(np.float64) @ truth[:3, :3].T
    return float(np.arccos(np.clip((np.trace(dR) - 1) / 2, -1, 1))), float(np.linalg.norm(T[:3, 3] - truth[:3, 3]))


def per_hypothesis(r, comp, starts):
    """n_inliers / dists_sum / matches / exclusion flag of every hypothesis from the reference's distances, by own code"""
    H = len(r['seeds']['view1'])
    n_inl, dsum, excl, matches = np.zeros(H, np.int32), np.zeros(H, np.float32), np.zeros(H, bool), []
    for h in range(H):
        p = comp['hyp_pair'][h]
        sl = slice(comp['pair_off'][p], comp['pair_off'][p + 1])
        d = r['dists'][starts[h]:starts[h + 1]]
        n_inl[h], dsum[h], m, conflict = walk(comp['pair_cand1'][sl], comp['pair_cand2'][sl], d)
        matches.append(m)
        excl[h] = conflict or bool(np.any(np.abs(d.astype(np.float64) - THRESHOLD) < NEAR))
    return n_inl, dsum, excl, matches


def best_per_pair(comp, n_inl, dsum):
    """cosypose_cext.cpp:187-210 restated: -> [(pair, hypothesis)] with hypothesis 0 never winning"""
    out = []
    for p in range(len(comp['pair_view1'])):
        best, bn, bd = -1, 0, np.float32(np.finfo(np.float32).max)
        for h in np.flatnonzero(comp['hyp_pair'] == p):
            if n_inl[h] >= N_MIN_INLIERS and (n_inl[h] > bn or (n_inl[h] == bn and dsum[h] < bd)):
                best, bn, bd = int(h), n_inl[h], dsum[h]
        if best > 0:
            out.append((p, best))
    return out


def store_inputs(out, prefix, scene):
    for k in SCENE_KEYS:
        out[prefix + 'in_' + k] = scene[k]


def store_stage(out, prefix, r):
    comp, starts = compact_tmatches(r['seeds'], r['tm'])
    for k in SEED_KEYS:
        out[prefix + 'seed_' + k] = np.asarray(r['seeds'][k], np.int32)
    for k, v in comp.items():
        out[prefix + 'tm_' + k] = v
    n_inl, dsum, excl, matches = per_hypothesis(r, comp, starts)
    winners = best_per_pair(comp, n_inl, dsum)
    inl = r['inliers']
    assert [h for _, h in winners] == list(inl['best_hypotheses']), 'own bookkeeping does not reproduce find_ransac_inliers'
    flat = [m for _, h in winners for m in matches[h]]
    assert [a for a, _ in flat] == list(inl['inlier_matches_cand1']) and [b for _, b in flat] == list(inl['inlier_matches_cand2'])
    share = excl.mean()
    print(f'  {prefix}: {len(excl)} hypotheses, {len(r["dists"])} scorings, {excl.sum()} left out of the n_inliers comparison ({share:.2%})')
    assert share <= 0.02, 'more than 2 % of the hypotheses are near a decision'
    sd = np.sort(r['sym_dists'], axis=1)
    gap = (sd[:, 1] - sd[:, 0]) if sd.shape[1] > 1 else np.full(len(sd), np.inf, np.float32)
    print(f'  {prefix}: {int((gap < 1e-5).sum())} hypotheses with a runner-up gap < 1e-5, {int((gap < NEAR).sum())} below 1e-4')
    out[prefix + 'TC1C2'] = r['TC1C2']; out[prefix + 'sym'] = r['sym']; out[prefix + 'gap'] = gap.astype(np.float32)
    out[prefix + 'sym_dists'] = r['sym_dists']; out[prefix + 'dists'] = r['dists']
    out[prefix + 'n_inliers'] = n_inl; out[prefix + 'dists_sum'] = dsum; out[prefix + 'excluded'] = excl
    out[prefix + 'best_hypotheses'] = np.asarray(inl['best_hypotheses'], np.int32)
    out[prefix + 'inlier_cand1'] = np.asarray(inl['inlier_matches_cand1'], np.int32)
    out[prefix + 'inlier_cand2'] = np.asarray(inl['inlier_matches_cand2'], np.int32)
    assert len(out[prefix + 'best_hypotheses']) >= 2 and 0 not in out[prefix + 'best_hypotheses']
    return comp, starts, n_inl


def compared(r):
    f, p, s = r['filtered'], r['pairs'], r['scene_infos']
    return (list(f.infos['cand_id']), partition(f.infos['obj_id']), sorted(zip(p.infos['view1'], p.infos['view2'])),
            sorted(zip(s['n_cand'], np.round(s['score'], 5), s['label'])))


def store_end_to_end(out, prefix, scene, r32, r64, with_seeds=True):
    assert compared(r32) == compared(r64), f'{prefix}: the reference in float32 and in float64 disagree on what the test compares'
    comp, starts = compact_tmatches(r32['seeds'], r32['tm'])
    n32 = per_hypothesis(r32, comp, starts)[0]
    n64 = per_hypothesis(r64, comp, starts)[0]
    if with_seeds:
        for k in SEED_KEYS:
            out[prefix + 'seed_' + k] = np.asarray(r32['seeds'][k], np.int32)
    f, s, inl = r32['filtered'], r32['scene_infos'], r32['inliers']
    out[prefix + 'e2e_cand_id'] = f.infos['cand_id'].values.astype(np.int64); out[prefix + 'e2e_obj_id'] = f.infos['obj_id'].values.astype(np.int64)
    out[prefix + 'e2e_info_n_cand'] = s['n_cand'].values.astype(np.int64); out[prefix + 'e2e_info_score'] = s['score'].values.astype(np.float64)
    out[prefix + 'e2e_info_label'] = np.array([int(l[4:]) - 1 for l in s['label'].values], np.int64)
    out[prefix + 'e2e_info_obj_id'] = s['obj_id'].values.astype(np.int64)
    best = np.asarray(inl['best_hypotheses'])
    assert np.array_equal(n32[best], n64[np.asarray(r64['inliers']['best_hypotheses'])]), f'{prefix}: winners\' n_inliers differ between float32 and float64'
    view_row = {v: n for n, v in enumerate(scene['cam_view_id'])}
    TCW = np.linalg.inv(scene['cam_TWC'])
    v1, v2, rot, trans = [], [], [], []
    for h in best:
        a, b = int(r32['seeds']['view1'][h]), int(r32['seeds']['view2'][h])
        truth = TCW[view_row[a]] @ scene['cam_TWC'][view_row[b]]
        rivals = np.flatnonzero((comp['hyp_pair'] == comp['hyp_pair'][h]) & (n32 >= n32[h]))
        errs = [pose_errors(r32['TC1C2'][j], truth) for j in rivals]
        v1.append(a); v2.append(b); rot.append(max(e[0] for e in errs)); trans.append(max(e[1] for e in errs))
    out[prefix + 'e2e_view1'] = np.array(v1, np.int64); out[prefix + 'e2e_view2'] = np.array(v2, np.int64)
    out[prefix + 'e2e_n_inliers'] = n32[best].astype(np.int32)
    out[prefix + 'e2e_rot_ceiling'] = np.array(rot); out[prefix + 'e2e_trans_ceiling'] = np.array(trans)
    truth_part = partition(scene['cand_obj_id'][out[prefix + 'e2e_cand_id']])
    print(f'  {prefix}: {len(f)} of {len(scene["cand_view_id"])} candidates kept, {len(s)} objects, {len(best)} view pairs; partition == ground truth: '
          f'{truth_part == partition(out[prefix + "e2e_obj_id"])}; worst ceilings {max(rot):.4f} rad, {max(trans):.4f} m')
    return truth_part == partition(out[prefix + 'e2e_obj_id'])


def main():
    R = reference()
    out = {}
    scene_a, scene_b, scene_d, scene_e = (syn.make_ba_scene(162, 6, 4, 8), syn.make_ba_scene(164, 12, 8, 8), syn.make_ba_scene(3, 10, 5, 8),
                                          syn.make_ba_scene(161, 3, 3, 8))
    f32, f64 = torch.float32, torch.float64

    print('a_: seed 162, 6 objects, 4 views, 2000 iterations')
    store_inputs(out, 'a_', scene_a)
    ra = run(R, scene_a, 2000, f32)
    comp, _, _ = store_stage(out, 'a_', ra)
    assert store_end_to_end(out, 'a_', scene_a, ra, run(R, scene_a, 2000, f64), with_seeds=False)
    sizes = np.diff(comp['pair_off'])
    assert np.all(sizes * (sizes - 1) <= 2000), 'a_: a view pair is not sampled exhaustively at 2000 iterations'

    print('b_: seed 164, 12 objects, 8 views, 50 iterations (stages)')
    store_inputs(out, 'b_', scene_b)
    store_stage(out, 'b_', run(R, scene_b, 50, f32))

    print('c_: seed 164 at 2000 iterations (end to end; inputs = b_)')
    rc = run(R, scene_b, 2000, f32)
    assert store_end_to_end(out, 'c_', scene_b, rc, run(R, scene_b, 2000, f64)), 'c_: the chain test needs the ground-truth partition'
    comp, _ = compact_tmatches(rc['seeds'], rc['tm'])
    sizes = np.diff(comp['pair_off'])
    assert np.all(sizes * (sizes - 1) <= 2000), 'c_: a view pair is not sampled exhaustively at 2000 iterations'

    print('d_: seed 3, 10 objects, 5 views, 2000 iterations (end to end)')
    store_inputs(out, 'd_', scene_d)
    store_end_to_end(out, 'd_', scene_d, run(R, scene_d, 2000, f32), run(R, scene_d, 2000, f64))

    print('k_: seed 162 with known camera poses (inputs = a_)')
    rk = run(R, scene_a, 1, f32, cameras=True)
    inl = rk['inliers']
    out['k_best_hypotheses'] = np.asarray(inl['best_hypotheses'], np.int32)
    out['k_view1'] = rk['pairs'].infos['view1'].values.astype(np.int64); out['k_view2'] = rk['pairs'].infos['view2'].values.astype(np.int64)
    out['k_TC1C2'] = rk['pairs'].TC1C2.numpy()
    out['k_cand_id'] = rk['filtered'].infos['cand_id'].values.astype(np.int64); out['k_obj_id'] = rk['filtered'].infos['obj_id'].values.astype(np.int64)
    for k in SEED_KEYS:
        out['k_seed_' + k] = np.asarray(rk['seeds'][k], np.int32)
    assert 0 not in out['k_best_hypotheses'] and len(out['k_best_hypotheses']) >= 3
    print(f'  k_: {len(rk["seeds"]["view1"])} hypotheses, {len(out["k_best_hypotheses"])} view pairs kept (hypothesis 0 never is), {len(out["k_cand_id"])} candidates')

    print('e_: seed 161, 3 objects, 3 views: nothing reaches n_min_inliers')
    store_inputs(out, 'e_', scene_e)
    re_ = run(R, scene_e, 2000, f32)
    assert len(re_['seeds']['view1']) > 0 and len(re_['inliers']['best_hypotheses']) == 0 and len(re_['filtered']) == 0
    for k in SEED_KEYS:
        out['e_seed_' + k] = np.asarray(re_['seeds'][k], np.int32)

    path = HERE / 'reference_golden_ransac.npz'
    save_npz(path, out)
    print('wrote', path.name, path.stat().st_size, 'bytes')


if __name__ == '__main__':
    main()
