#!/usr/bin/env python3
"""Generate tests/golden/reference_golden_ransac_edges.npz: the REFERENCE's own multi-view matching functions on the edge inputs of
tests/test_ransac_kernels.py -- estimate_camera_poses and score_tmatches (cosypose/multiview/ransac.py:19-47, :67-73) in torch
FLOAT64 on one thread, and the compiled find_ransac_inliers (cosypose/csrc/cosypose_cext.cpp:107-216, built into oracle/_ref by
oracle/build_ref.sh).  tests/ransac_ref.py (the yardstick of the GPU tests) is held to these values on the CPU.
Run in the build container only:   python tests/golden/generate_golden_ransac_edges.py

The inputs come from the seeded functions below (numpy + cosypose_amd.synthetic; the test imports this file and calls them); the
fixture holds the reference's OUTPUTS only.  Shims as in generate_golden_ransac.py.  No reference source is copied: the reference
is imported and executed in place.

  h_<case>_   hypotheses: TC1C2, the (H,S) distance of every symmetry of match 1's label (the reference's distance function once per
              symmetry index, asserted to explain the reference's TC1C2), the chosen symmetry
  s_          computed distances: score_tmatches for the first SCORE_FIXTURE_HYPS hypotheses of every view pair of the 30-object scene
  w_<case>_   given distances: find_ransac_inliers on the whole problem (best hypotheses, inlier matches) and, for EVERY hypothesis,
              its walk: the hypothesis is passed as id 1 next to an empty hypothesis 0 of another view pair, with n_min_inliers = 0
  b_<case>_   best hypothesis per view pair on crafted tables: best hypotheses and inlier matches
The hypotheses of the s_ block are built by the twin (score_scene takes its float32 TC1C2 from ransac_ref.ref_hypotheses), so those
INPUTS follow the code the fixture holds: a change of the twin that moves them makes test_twin_vs_reference fail against the stored
distances until the fixture is regenerated, which is the intended alarm.
find_ransac_inliers returns no dists_sum: the float32 sums are held through the winners they decide (the b_ cases tie on them).
"""
import pathlib
import sys

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
REPO = HERE.parent.parent
OUT = HERE / 'reference_golden_ransac_edges.npz'

F32 = np.float32
THR = F32(0.02)
LENGTHS = (1, 2, 127, 128, 129, 257, 1000, 4096)           # list lengths around the 128-slot sort, the 128-thread loops and the limit
SCORE_FIXTURE_HYPS = 2

# name: (S, n_sym per label, P, H)
HYP_CASES = {
    'S1_H1': (1, [1], 1, 1), 'S1_H257': (1, [1], 1, 257),                                  # G = 1
    'S3': (3, [1, 2, 3], 8, 65),                                                           # G = 4, one idle lane
    'S5': (5, [1, 5, 2, 4], 37, 63),                                                       # G = 8, three idle lanes
    'S33': (33, [33, 7], 3, 9),                                                            # G = 64, 31 idle lanes
    'S64_H3': (64, [64, 1, 33, 2], 8, 3), 'S64_H4': (64, [64, 1, 33, 2], 8, 4), 'S64_H5': (64, [64, 1, 33, 2], 8, 5),
    'tie': (4, [4, 4], 8, 12),                                                             # S_2 a bit-identical copy of S_1
}


def _rot(rs):
    q, r = np.linalg.qr(rs.randn(3, 3))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def _poses(rs, n):
    """random rotations at 0.3-1.5 m"""
    T = np.tile(np.eye(4), (n, 1, 1))
    for i in range(n):
        T[i, :3, :3] = _rot(rs)
        z = rs.uniform(0.3, 1.5)
        T[i, :3, 3] = (rs.uniform(-0.2, 0.2) * z, rs.uniform(-0.2, 0.2) * z, z)
    return T.astype(F32)


def mesh_tables(rs, S, n_sym, P):
    """points random in 3-12 cm boxes; symmetries = rotations about z by 2 pi k / n_sym, identity-padded to S"""
    n_mesh = len(n_sym)
    pts = (rs.uniform(-1, 1, (n_mesh, P, 3)) * rs.uniform(0.015, 0.06, (n_mesh, 1, 3))).astype(F32)
    sym = np.tile(np.eye(4, dtype=F32), (n_mesh, S, 1, 1))
    for m in range(n_mesh):
        for k in range(1, n_sym[m]):
            a = 2 * np.pi * k / n_sym[m]
            sym[m, k, :3, :3] = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], F32)
    return pts, sym, np.array(n_sym, np.int32)


def hyp_case(name):
    """float32 inputs of one hypotheses case: 6 candidates per label; match 1's label cycles through the table; every fourth seed's
    two matches are the same pair.  'tie': rows 1 and 2 of both tables are the same bits, and match 2 of six seeds (`planted`) is placed
    at TC1Oa S_1 inv(TC2Ob) TC2Od, so that symmetries 1 and 2 share the minimum."""
    S, n_sym, P, H = HYP_CASES[name]
    rs = np.random.RandomState(1000 + list(HYP_CASES).index(name))
    pts, sym, n_sym = mesh_tables(rs, S, n_sym, P)
    n_mesh = len(n_sym)
    n_cand = 6 * n_mesh
    cand_mesh = (np.arange(n_cand) % n_mesh).astype(np.int32)
    poses = _poses(rs, n_cand)
    i = np.arange(H)
    a = (5 * i) % n_cand
    g = (7 * i + 1) % n_cand
    b = (a + n_mesh * rs.randint(1, 6, H)) % n_cand           # same label as a
    d = (g + n_mesh * rs.randint(1, 6, H)) % n_cand
    same = i % 4 == 1
    g[same], d[same] = a[same], b[same]
    planted = np.zeros(0, np.int64)
    if name == 'tie':
        sym[:, 2] = sym[:, 1]
        w = lambda T: T.astype(np.float64)
        extra = []
        planted = np.flatnonzero(~same)[:6]
        for n, h in enumerate(planted):
            extra.append((w(poses[a[h]]) @ w(sym[cand_mesh[a[h]], 1]) @ np.linalg.inv(w(poses[b[h]])) @ w(poses[d[h]])).astype(F32))
            cand_mesh = np.append(cand_mesh, cand_mesh[d[h]]).astype(np.int32)
            g[h] = n_cand + n
        poses = np.concatenate([poses, np.array(extra)])
    seeds = np.stack([a, b, g, d], 1).astype(np.int32)
    return dict(pts=pts, sym=sym, n_sym=n_sym, poses=poses, cand_mesh=cand_mesh, seeds=seeds, planted=planted)


# ---- given distances ---------------------------------------------------------------------------------------------------------------
def walk_values(signed):
    v = [0.0, 0.0025, 0.01, 0.0175, THR, np.nextafter(THR, F32(np.inf)), np.inf, np.nan]
    return np.array(v + ([-0.0, -0.005, -1.0] if signed else []), F32)


def _problem(pair_c1, pair_c2, hyp_pair, rows, n_min):
    """lists of (cand1, cand2) per pair, each hypothesis's pair and distance row -> the compact layout + the float32 table"""
    sizes = [len(c) for c in pair_c1]
    return dict(pair_off=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), pair_c1=np.concatenate(pair_c1).astype(np.int32),
                pair_c2=np.concatenate(pair_c2).astype(np.int32), hyp_pair=np.asarray(hyp_pair, np.int32),
                pair_view1=np.zeros(len(sizes), np.int32), pair_view2=np.arange(1, len(sizes) + 1, dtype=np.int32),
                dists=np.concatenate(rows).astype(F32) if len(rows) else np.zeros(0, F32), thr=THR, n_min=int(n_min))


def walk_case(signed):
    """One launch, one view pair per list length, three hypotheses per pair (ids interleaved); distances drawn from walk_values; the
    candidates of a list of n matches are drawn from min(n, 48 + n / 16) per side, with ids that are not their ranks."""
    rs = np.random.RandomState(77 + int(signed))
    vals = walk_values(signed)
    c1, c2 = [], []
    for p, n in enumerate(LENGTHS):
        k = min(n, 48 + n // 16)
        c1.append(10000 * (p + 1) + 2 * rs.randint(k, size=n))
        c2.append(20000 * (p + 1) + 3 * rs.randint(k, size=n))
    hyp_pair = np.tile(np.arange(len(LENGTHS)), 3)
    rows = [vals[rs.randint(len(vals), size=LENGTHS[p])] for p in hyp_pair]
    return _problem(c1, c2, hyp_pair, rows, 1)


# ---- best hypothesis per pair on crafted tables ----------------------------------------------------------------------------------------
BEST_L = 8          # disjoint matches per pair: every inlier is accepted, a row's (n_inliers, dists_sum) is what was written into it
BEST_CASES = ('main', 'n_min0', 'zero_unique', 'zero_tied')


def _row(n, mm=None):
    """n inliers of mm[i] millimetres (default 1 mm each), the rest +inf"""
    r = np.full(BEST_L, np.inf, F32)
    r[:n] = F32(0.001) * np.asarray(mm if mm is not None else np.ones(n), F32)
    return r


def best_case(name):
    """'main' (n_min_inliers 3): pairs with 0, 1, 2, 127, 128, 129 and 4 x 300 hypotheses, ids dealt round-robin over the pairs.  The
    one hypothesis of pair 1 has exactly 3 inliers (wins), both of pair 2 have 2 (no winner); the others are random rows of 0-7
    inliers of 1-3 mm (exact ties abound); each 300-pair holds the unique best row (8 inliers) twice, at positions 5 and 5 + 1 / 127
    / 128 / 129 of the pair.  The small cases: see the rows."""
    rs = np.random.RandomState(5)
    if name == 'main':
        per_pair = [0, 1, 2, 127, 128, 129, 300, 300, 300, 300]
        rows = {p: [_row(n, rs.randint(1, 4, n)) for n in rs.randint(0, BEST_L, per_pair[p])] for p in range(len(per_pair))}
        rows[1] = [_row(3)]
        rows[2] = [_row(2), _row(2, [1, 2])]
        rows[3][0] = _row(0)                                        # becomes hypothesis 0
        for p, dist in zip((6, 7, 8, 9), (1, 127, 128, 129)):
            rows[p][5] = rows[p][5 + dist] = _row(BEST_L)
        order = sorted(((pos, (p - 3) % len(per_pair), p) for p in rows for pos in range(len(rows[p]))))
        hyp_pair, table, n_min = [p for _, _, p in order], [rows[p][pos] for pos, _, p in order], 3
    else:
        n_min = 0 if name == 'n_min0' else 3
        hyp_pair = dict(n_min0=[0, 1, 0])[name] if name == 'n_min0' else [0, 1, 0, 1]
        table = dict(n_min0=[_row(5), _row(0), _row(2)], zero_unique=[_row(5), _row(4), _row(3), _row(2)],
                     zero_tied=[_row(5), _row(4), _row(5), _row(2)])[name]
        per_pair = [2, 2]
    c1 = [100 * p + np.arange(BEST_L) for p in range(len(per_pair))]
    c2 = [100 * p + 50 + np.arange(BEST_L) for p in range(len(per_pair))]
    return _problem(c1, c2, hyp_pair, table, n_min)


# ---- computed distances --------------------------------------------------------------------------------------------------------------
def score_scene(n_objects, n_views, seed=11):
    """A make_ba_scene scene (8 box corners) whose candidates are doubled: the first half of each view's candidates is copied with 3 mm
    of translation noise (what makes conflicts).  Tentative matches = same label, different views, per ordered view pair, cand1-major;
    the lists are cut to lengths around the sort sizes.  Per pair 8 hypotheses from seeds whose two matches join the same true
    objects and 4 from random seeds, TC1C2 from ransac_ref.ref_hypotheses narrowed to float32."""
    from cosypose_amd import synthetic as syn
    import ransac_ref as rr
    sc = syn.make_ba_scene(seed, n_objects, n_views, 8)
    rs = np.random.RandomState(seed + 1)
    view, obj, label, poses = sc['cand_view_id'], sc['cand_obj_id'], sc['cand_label_id'], sc['cand_poses']
    dup = np.concatenate([np.flatnonzero(view == v)[:(int((view == v).sum()) + 1) // 2] for v in sc['cam_view_id']])
    copies = poses[dup].copy()
    copies[:, :3, 3] += rs.randn(len(dup), 3) * 0.003
    view, obj, label, poses = np.concatenate([view, view[dup]]), np.concatenate([obj, obj[dup]]), np.concatenate([label, label[dup]]), np.concatenate([poses, copies])
    order = np.argsort(view, kind='stable')                    # the copies next to their view
    view, obj, label, poses = view[order], obj[order], label[order].astype(np.int32), poses[order].astype(F32)
    cuts = (None, 257, 129, 128, 127, None) if n_views == 3 else (None, 1000)
    pts, sym = sc['pts'].astype(F32), sc['sym'].astype(F32)
    c1, c2, hyp_pair, seeds = [], [], [], []
    pairs = [(a, b) for a in sc['cam_view_id'] for b in sc['cam_view_id'] if a != b]
    for p, (va, vb) in enumerate(pairs):
        n, m = np.nonzero((label[:, None] == label[None, :]) & (view[:, None] == va) & (view[None, :] == vb))
        cut = cuts[p % len(cuts)]
        n, m = n[:cut], m[:cut]
        c1.append(n); c2.append(m)
        true = np.flatnonzero(obj[n] == obj[m])
        for k in range(12):
            while True:
                i, j = rs.choice(true, 2) if k < 8 else rs.randint(len(n), size=2)
                if i != j and (k >= 8 or obj[n[i]] != obj[n[j]]):
                    break
            seeds.append((n[i], m[i], n[j], m[j])); hyp_pair.append(p)
    seeds = np.array(seeds, np.int32)
    TC1C2 = rr.ref_hypotheses(poses, label, pts, sym, sc['n_sym'], seeds)['TC1C2'].astype(F32)
    out = _problem(c1, c2, hyp_pair, [], 3)
    out.update(poses=poses, cand_mesh=label, pts=pts, sym=sym, n_sym=sc['n_sym'].astype(np.int32), TC1C2=TC1C2, cand_view=view, cand_obj=obj,
               pair_view1=np.array([a for a, _ in pairs], np.int32), pair_view2=np.array([b for _, b in pairs], np.int32))
    del out['dists']
    return out


def hyp_rows(pr):
    """[(hypothesis, slice of its pair's match list, slice of its row in the expanded distance table)]"""
    sizes = np.diff(pr['pair_off'])[pr['hyp_pair']]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return [(h, slice(int(pr['pair_off'][p]), int(pr['pair_off'][p + 1])), slice(int(off[h]), int(off[h + 1]))) for h, p in enumerate(pr['hyp_pair'])]


def score_fixture_hyps(pr):
    """the hypotheses of the s_ fixture: the first SCORE_FIXTURE_HYPS of every view pair"""
    return [h for p in range(len(pr['pair_view1'])) for h in np.flatnonzero(pr['hyp_pair'] == p)[:SCORE_FIXTURE_HYPS]]


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
def main():
    for p in (REPO, HERE.parent, HERE):            # the package, ransac_ref, the other generators; a test that imports this file has its own path
        if str(p) not in sys.path:
            sys.path.insert(0, str(p))
    import torch
    from generate_golden_ransac import reference
    from generate_golden_ba import save_npz
    R = reference()
    rs_mod, sdist, cext = R['ransac'], R['sdist'], R['cext']
    f64 = torch.float64
    out = {}

    def mesh_db_of(c):
        labels = np.array([f'obj_{i:06d}' for i in range(1, len(c['n_sym']) + 1)])
        infos = {l: dict(label=l, n_sym=int(c['n_sym'][i])) for i, l in enumerate(labels)}
        return labels, R['BatchedMeshes'](infos, labels, torch.as_tensor(c['pts']).to(f64), torch.as_tensor(c['sym']).to(f64))

    with torch.no_grad():
        for name in HYP_CASES:
            c = hyp_case(name)
            labels, mesh_db = mesh_db_of(c)
            poses = torch.as_tensor(c['poses']).to(f64)
            a, b, g, d = (c['seeds'][:, i].astype(np.int64) for i in range(4))
            l_ab, l_gd = labels[c['cand_mesh'][a]], labels[c['cand_mesh'][g]]
            TC1C2 = rs_mod.estimate_camera_poses(poses[a], poses[b], l_ab, poses[g], poses[d], l_gd, mesh_db)
            S = c['sym'].shape[1]
            mesh_row, n_sym = c['cand_mesh'][a].astype(np.int64), c['n_sym'][c['cand_mesh'][a]]
            T_b_inv = R['invert_T'](poses[b])
            rows = np.full((len(a), S), np.inf)
            for k in range(S):
                dk, _ = sdist.symmetric_distance_batched_fast(poses[g], (poses[a] @ mesh_db.symmetries[mesh_row, k] @ T_b_inv) @ poses[d], l_gd, mesh_db)
                rows[:, k] = np.where(k < n_sym, dk.numpy(), np.inf)
            chosen = rows.astype(F32).argmin(1)
            assert torch.equal(poses[a] @ mesh_db.symmetries[mesh_row, chosen] @ T_b_inv, TC1C2), f'{name}: the rows do not explain the reference\'s choice'
            out[f'h_{name}_TC1C2'], out[f'h_{name}_rows'], out[f'h_{name}_best'] = TC1C2.numpy(), rows, chosen.astype(np.int32)
            print(f'h_{name}: {len(a)} seeds, chosen symmetries {np.bincount(chosen).tolist()[:8]}')

        pr = score_scene(30, 3)
        labels, mesh_db = mesh_db_of(pr)
        poses = torch.as_tensor(pr['poses']).to(f64)
        rows, dd = hyp_rows(pr), []
        for h in score_fixture_hyps(pr):
            _, sl, _ = rows[h]
            c1, c2 = pr['pair_c1'][sl].astype(np.int64), pr['pair_c2'][sl].astype(np.int64)
            T = torch.as_tensor(pr['TC1C2'][h]).to(f64)[None].expand(len(c1), 4, 4)
            dd.append(rs_mod.score_tmatches(poses[c1], poses[c2], T, labels[pr['cand_mesh'][c1]], mesh_db).numpy())
        out['s_dists'] = np.concatenate(dd)
        print(f's_: {len(dd)} hypotheses, {len(out["s_dists"])} distances')

    def run_inliers(prefix, pr, per_hypothesis):
        rows = hyp_rows(pr)
        v1, v2 = pr['pair_view1'][pr['hyp_pair']], pr['pair_view2'][pr['hyp_pair']]
        hyp = np.concatenate([np.full(sl.stop - sl.start, h, np.int32) for h, sl, _ in rows] + [np.zeros(0, np.int32)])
        c1 = np.concatenate([pr['pair_c1'][sl] for _, sl, _ in rows] + [np.zeros(0, np.int32)])
        c2 = np.concatenate([pr['pair_c2'][sl] for _, sl, _ in rows] + [np.zeros(0, np.int32)])
        inl = cext.find_ransac_inliers(v1.astype(np.int32), v2.astype(np.int32), hyp, c1, c2, pr['dists'], float(pr['thr']), pr['n_min'])
        out[prefix + 'best'] = np.asarray(inl['best_hypotheses'], np.int32)
        out[prefix + 'c1'], out[prefix + 'c2'] = np.asarray(inl['inlier_matches_cand1'], np.int32), np.asarray(inl['inlier_matches_cand2'], np.int32)
        print(f'{prefix}: best {out[prefix + "best"].tolist()}, {len(out[prefix + "c1"])} inlier matches')
        if per_hypothesis:
            count, m1, m2 = [], [], []
            for h, sl, dsl in rows:
                n = sl.stop - sl.start
                one = cext.find_ransac_inliers(np.array([-1, 0], np.int32), np.array([-1, 1], np.int32), np.ones(n, np.int32), pr['pair_c1'][sl],
                                               pr['pair_c2'][sl], pr['dists'][dsl], float(pr['thr']), 0)
                assert list(one['best_hypotheses']) == [1]
                count.append(len(one['inlier_matches_cand1'])); m1.append(np.asarray(one['inlier_matches_cand1'], np.int32)); m2.append(np.asarray(one['inlier_matches_cand2'], np.int32))
            out[prefix + 'walk_n'], out[prefix + 'walk_c1'], out[prefix + 'walk_c2'] = np.array(count, np.int32), np.concatenate(m1), np.concatenate(m2)

    for signed in (False, True):
        run_inliers(f'w_{"signed" if signed else "plain"}_', walk_case(signed), True)
    for name in BEST_CASES:
        run_inliers(f'b_{name}_', best_case(name), False)

    save_npz(OUT, out)
    print('wrote', OUT.name, OUT.stat().st_size, 'bytes')
    assert OUT.stat().st_size < 200 * 1024


if __name__ == '__main__':
    main()
