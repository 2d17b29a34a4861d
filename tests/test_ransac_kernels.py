"""The three kernels of csrc/kernels_ransac.hip (hypotheses, score + inliers, best per view pair) against float64 at the shapes
where they take another path.

tests/test_multiview_matching.py runs one shape family (P = 8, S = 4, lists of 7-25 matches, at most 132 hypotheses per pair): the
lane group is always 4, every 128-thread loop runs once, the sort has one size and the "already used" sets one word.  Here:
  * hypotheses at G = 1, 4, 8, 64 with idle lanes, partial / full / overfull workgroups, pinned ties, invalid seeds (raw ABI);
  * score + walk on GIVEN distances (exact: no rounding involved) at list lengths 1 .. 4096 in one launch, distances drawn from a
    handful of values so that exact ties are the rule, with -0 and negative values;
  * score on COMPUTED distances on scenes with doubled candidates (hundreds of matches per list, dozens of conflicts);
  * best per view pair on crafted tables: 0 .. 300 hypotheses per pair, planted exact ties 1 / 127 / 128 / 129 positions apart.
The yardstick is tests/ransac_ref.py, numpy twins restated from the reference's text; test_twin_vs_reference holds them to the
reference's own float64 run (tests/golden/reference_golden_ransac_edges.npz, written by generate_golden_ransac_edges.py) and
test_cases_discriminate shows that eight plausible kernel mistakes would change what the cases expect.  Both need no GPU.

Bounds.  Decisions (indices, counts, match lists, float32 sums) are compared exactly.  Real values are judged per item, absolute
in metres, against float64 on the same float32 inputs, by at most 3 x the worst figure measured on an MI355X and never above the
project's ceiling DIST_TOL = 1e-5 (numpy float32 against float64 on such scenes: 1.2e-7 - 1.5e-7):
    quantity                                         worst measured                  bound
    hypotheses, distance of every symmetry           3.21e-7 (S = 64, 3 seeds)       ROW_TOL   = 9e-7
    hypotheses, TC1C2 entries                        2.03e-7 (S = 1, 257 seeds)      TC_TOL    = 6e-7
    score, computed distances                        1.37e-7 (60 objects, 2 views)   SCORE_TOL = 4e-7
The hypotheses' distances are between random poses, 0.5 - 3 m apart (one float32 ulp of 2 m is 2.4e-7); the scored ones are
centimetres between poses at 0.9 m.

The inner argmin (which symmetry of the OTHER label explains a distance) is not determined where two mean squared costs agree to
rounding, so a distance is accepted if it is within the bound of the float64 distance of ANY admissible symmetry: one whose
float64 cost lies within the float32 cost error of the minimum.  That error, to first order in u = 2^-24:
    a transformed point goes through at most five float32 stages (invert, three 4x4 products, the point transform), each entry a
    dot product of <= 4 terms: <= 4 u sum|a||b| <= 4 sqrt(3) u L per stage and component, where L = the translations involved + the
    mesh radius bounds every coordinate; an earlier stage's rotation error times a later translation doubles it: ~70 u L; the other
    point (two stages) ~28 u L; as a vector (x sqrt(3)) the difference D of the two points is off by e <= 173 u L -> E_DELTA = 256 u L.
    |D|^2 is then off by 2 |D| e + e^2 and its three roundings; the sum over P points adds (P - 1) u, the division one more:
        |cost32 - cost64| <= 2 dist64 e + e^2 + (P + 3) u cost64        (dist64 = mean |D|, cost64 = mean |D|^2)
A symmetry k is admissible when cost64[k] - min cost64 <= band[k] + band[argmin].  Symmetries whose float64 distances are the same
bits (identity padding, a copied table row) count as one; at least 95 % of all entries have a single admissible symmetry (asserted).

Every test prints its figures before it asserts (pytest -s shows them).
"""
import functools
import importlib.util
import pathlib

import numpy as np
import pytest

import ransac_ref as rr

REPO = pathlib.Path(__file__).resolve().parent.parent
gpu = pytest.mark.gpu

U = 2.0 ** -24
F32 = np.float32
DIST_TOL = 1e-5           # the project's ceiling for float32 distances (metres)
FP64_TOL = 1e-13          # twin against the reference in float64: rounding over a few dozen operations
E_DELTA = 256             # x u L: the float32 error of a point difference (module docstring)
# measured on an MI355X (worst over all cases) -> bound = at most 3 x, below DIST_TOL
ROW_TOL = 9e-7            # hypotheses, distance of every symmetry: measured 3.21e-7 (x 3 = 9.63e-7)
TC_TOL = 6e-7             # hypotheses, TC1C2 entries: measured 2.03e-7 (x 3 = 6.09e-7)
SCORE_TOL = 4e-7          # score, computed distances: measured 1.37e-7 (x 3 = 4.10e-7)
assert max(ROW_TOL, TC_TOL, SCORE_TOL) <= DIST_TOL


@functools.lru_cache(None)
def E():
    spec = importlib.util.spec_from_file_location('generate_golden_ransac_edges', REPO / 'tests' / 'golden' / 'generate_golden_ransac_edges.py')
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@functools.lru_cache(None)
def fixture():
    return dict(np.load(E().OUT, allow_pickle=False))


def bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32)


# ---- admissible symmetries -----------------------------------------------------------------------------------------------------------
def admissible(dist, cost, L, P):
    """dist, cost (..., K) float64 of every symmetry, L (...) the coordinate scale -> bool (..., K) (module docstring)"""
    e = E_DELTA * U * np.asarray(L, np.float64)[..., None]
    band = 2 * dist * e + e * e + (P + 3) * U * cost
    kmin = cost.argmin(-1)[..., None]
    return cost - np.take_along_axis(cost, kmin, -1) <= band + np.take_along_axis(band, kmin, -1)


def judged(got, dist, adm):
    """-> (error of `got` against the nearest admissible float64 distance, whether all admissible distances are the same bits)"""
    err = np.where(adm, np.abs(np.asarray(got, np.float64)[..., None] - dist), np.inf).min(-1)
    lo, hi = np.where(adm, dist, np.inf).min(-1), np.where(adm, dist, -np.inf).max(-1)
    return err, lo == hi


def norms(T):
    return np.linalg.norm(np.asarray(T, np.float64)[..., :3, 3], axis=-1)


# ---- expectations (CPU, computed once) --------------------------------------------------------------------------------------------------
def hyp_expect_of(c):
    t = rr.ref_hypotheses(c['poses'], c['cand_mesh'], c['pts'], c['sym'], c['n_sym'], c['seeds'])
    a, b, g, d = c['seeds'].T
    radius = np.linalg.norm(c['pts'].astype(np.float64), axis=-1).max(1)
    L = norms(c['poses'][a]) + norms(c['poses'][b]) + norms(c['poses'][g]) + norms(c['poses'][d]) + radius[c['cand_mesh'][g]]
    finite = np.isfinite(t['rows'])
    cost = np.where(np.isfinite(t['cost']), t['cost'], np.finfo(np.float64).max)      # rows past n_sym: judged by `finite` alone
    dist0 = np.where(np.isfinite(t['dist']), t['dist'], 0.0)
    t.update(L=L, finite=finite, dist0=dist0, adm=admissible(dist0, cost, L[:, None], c['pts'].shape[1]))
    return t


@functools.lru_cache(None)
def hyp_case(name):
    return E().hyp_case(name)


@functools.lru_cache(None)
def hyp_expect(name):
    return hyp_expect_of(hyp_case(name))


@functools.lru_cache(None)
def single_admissible_share():
    """share of all row entries of all hypotheses cases that have one admissible symmetry (CPU); asserted >= 95 %"""
    one = total = 0
    for name in E().HYP_CASES:
        t = hyp_expect(name)
        _, single = judged(np.where(t['finite'], t['rows'], 0.0), t['dist0'], t['adm'])
        one += int(single[t['finite']].sum()); total += int(t['finite'].sum())
    return one / total, total


def inliers_expect_of(pr, skip0=True, n_min=None):
    return rr.find_inliers(pr['hyp_pair'], pr['pair_off'], pr['pair_c1'], pr['pair_c2'], pr['dists'], pr['thr'], pr['n_min'] if n_min is None else n_min, skip0)


@functools.lru_cache(None)
def walk_case(signed):
    return E().walk_case(signed)


@functools.lru_cache(None)
def walk_expect(signed):
    """the twin's result + the preconditions of the given-distance case, from the CPU alone"""
    pr = walk_case(signed)
    want = inliers_expect_of(pr)
    for p, n in enumerate(E().LENGTHS):
        sl = slice(pr['pair_off'][p], pr['pair_off'][p + 1])
        hyps = np.flatnonzero(pr['hyp_pair'] == p)
        if n >= 128:
            assert want['skipped'][hyps].max() >= 10, (n, want['skipped'][hyps])
        if n >= 129:
            c1, c2 = pr['pair_c1'][sl], pr['pair_c2'][sl]
            (u1, r1), (u2, r2) = np.unique(c1, return_inverse=True), np.unique(c2, return_inverse=True)
            assert len(u1) >= 33 and len(u2) >= 33
            deep = 0
            for h in hyps:
                _, _, matches, _ = rr.walk(c1, c2, pr['dists'][E().hyp_rows(pr)[h][2]], pr['thr'])
                deep += sum(1 for a, b in matches if np.searchsorted(u1, a) >= 32 and np.searchsorted(u2, b) >= 32)
            assert deep >= 1, f'list of {n}: no accepted inlier with both ranks >= 32'
    return want


@functools.lru_cache(None)
def best_case(name):
    return E().best_case(name)


@functools.lru_cache(None)
def score_scene(n_objects, n_views):
    return E().score_scene(n_objects, n_views)


def score_expect(pr, hyps=None):
    """the twin's distances of the hypotheses `hyps` (default all) -> [(h, list slice, table slice, d, dist (n,S), cost (n,S), L)]"""
    out = []
    radius = np.linalg.norm(pr['pts'].astype(np.float64), axis=-1).max(1)
    for h, sl, dsl in E().hyp_rows(pr):
        if hyps is not None and h not in hyps:
            continue
        c1, c2 = pr['pair_c1'][sl], pr['pair_c2'][sl]
        d, dist, cost = rr.ref_score(pr['poses'], pr['cand_mesh'], pr['pts'], pr['sym'], pr['TC1C2'][h], c1, c2)
        L = norms(pr['TC1C2'][h]) + norms(pr['poses'][c1]) + norms(pr['poses'][c2]) + radius[pr['cand_mesh'][c1]]
        out.append((h, sl, dsl, d, dist, cost, L))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# non-GPU: the twin against the reference, and the cases against the mistakes they are meant to catch
# ---------------------------------------------------------------------------------------------------------------------------------------
RESIDUE = 1e-6            # x L: below this a distance is a rounding residue of metre-sized coordinates, not a length


def rel(got, want, L):
    """per item |got - want| / |want|.  Only a distance that is a rounding residue of the coordinates it was formed from (a seed whose
    two matches are the same pair, an exact true match: want < RESIDUE x L, in practice below 1e-7 m against L of metres) is judged
    relative to that coordinate scale L instead: its own bits are noise in the reference as here.  -> (worst, residue items)"""
    got, want, L = np.asarray(got, np.float64), np.asarray(want, np.float64), np.broadcast_to(np.asarray(L, np.float64), np.shape(want))
    residue = np.abs(want) < RESIDUE * L
    err = np.abs(got - want) / np.where(residue, L, np.abs(want))
    return (float(err.max()) if err.size else 0.0), int(residue.sum())


def rel_pose(got, want):
    """per pose max |got - want| / max |want| of that pose"""
    a, b = np.asarray(got, np.float64).reshape(-1, 16), np.asarray(want, np.float64).reshape(-1, 16)
    return float((np.abs(a - b).max(1) / np.abs(b).max(1)).max()) if len(b) else 0.0


def test_twin_vs_reference():
    """ransac_ref.py against the reference's own run on the edge inputs: real values (every symmetry's distance, TC1C2, the computed
    distances of the 30-object scene) within 1e-13 relative per item in float64 (a distance relative to itself, see rel(); a pose
    relative to its largest entry); chosen symmetries, best hypotheses, inlier-match
    lists of the winners AND the walk of every single hypothesis of the given-distance cases (with -0 and negative distances)
    exactly.  The reference's find_ransac_inliers returns no dists_sum: the float32 sums are held through the winners they decide
    (the crafted tables tie on them)."""
    g = fixture()
    worst = {}
    for name in E().HYP_CASES:
        c, t = hyp_case(name), hyp_expect(name)
        want_rows = g[f'h_{name}_rows']
        assert np.array_equal(np.isfinite(want_rows), t['finite'])
        e_rows, n_res = rel(t['rows'][t['finite']], want_rows[t['finite']], np.broadcast_to(t['L'][:, None], want_rows.shape)[t['finite']])
        # a seed whose two matches are the same pair gives EVERY symmetry the distance 0 up to float64 rounding: there the last bit
        # picks the symmetry, in the reference as here, and the index is held only to "a minimum of the row within FP64_TOL"
        clear = (t['gap'] > 1e-12 * t['L']) | (t['gap'] == 0)             # gap == 0: two rows of the same bits, the first index is determined
        ref_best = g[f'h_{name}_best']
        e_tc = rel_pose(t['TC1C2'][clear], g[f'h_{name}_TC1C2'][clear])
        excess = (t['rows'][np.arange(len(ref_best)), ref_best] - t['rows'].min(1)) / t['L']
        worst[name] = (e_rows, e_tc)
        print(f'  hypotheses {name}: rows {e_rows:.3g} ({n_res} residues of {int(t["finite"].sum())})  TC1C2 {e_tc:.3g}  seeds decided by rounding {int((~clear).sum())} / {len(clear)}')
        assert e_rows < FP64_TOL and e_tc < FP64_TOL
        assert np.array_equal(t['best'][clear], ref_best[clear]) and np.all(excess < FP64_TOL)
    pr = score_scene(30, 3)
    got = np.concatenate([d for _, _, _, d, _, _, _ in score_expect(pr, set(E().score_fixture_hyps(pr)))])
    Ls = np.concatenate([L for *_, L in score_expect(pr, set(E().score_fixture_hyps(pr)))])
    e_score, n_res = rel(got, g['s_dists'], Ls)
    print(f'  score: {len(got)} distances {e_score:.3g} ({n_res} residues)')
    assert len(got) == len(g['s_dists']) and e_score < FP64_TOL
    for signed in (False, True):
        pr, want, prefix = walk_case(signed), walk_expect(signed), f'w_{"signed" if signed else "plain"}_'
        assert np.array_equal(want['best_hypotheses'], g[prefix + 'best'])
        assert np.array_equal(want['inlier_matches_cand1'], g[prefix + 'c1']) and np.array_equal(want['inlier_matches_cand2'], g[prefix + 'c2'])
        assert np.array_equal(want['n_inliers'], g[prefix + 'walk_n'])
        m1, m2 = [], []
        for h, sl, dsl in E().hyp_rows(pr):
            _, _, matches, _ = rr.walk(pr['pair_c1'][sl], pr['pair_c2'][sl], pr['dists'][dsl], pr['thr'])
            m1 += [a for a, _ in matches]; m2 += [b for _, b in matches]
        assert np.array_equal(m1, g[prefix + 'walk_c1']) and np.array_equal(m2, g[prefix + 'walk_c2'])
        print(f'  {prefix}: {len(want["best_hypotheses"])} winners, {len(m1)} walked matches equal')
    for name in E().BEST_CASES:
        want = inliers_expect_of(best_case(name))
        assert np.array_equal(want['best_hypotheses'], g[f'b_{name}_best'])
        assert np.array_equal(want['inlier_matches_cand1'], g[f'b_{name}_c1']) and np.array_equal(want['inlier_matches_cand2'], g[f'b_{name}_c2'])


def test_case_preconditions():
    """From the CPU alone: >= 95 % of all hypotheses row entries have a single admissible symmetry; the given-distance lists reach the
    second word of both `used` sets and skip >= 10 conflicts per list of >= 128; the planted rows of the best cases win."""
    share, total = single_admissible_share()
    print(f'  single admissible symmetry: {share:.4f} of {total} row entries')
    assert share >= 0.95
    for signed in (False, True):
        want = walk_expect(signed)
        print(f'  given distances ({"signed" if signed else "plain"}): n_inliers up to {want["n_inliers"].max()}, skipped up to {want["skipped"].max()}')
    t, planted = hyp_expect('tie'), hyp_case('tie')['planted']
    assert len(planted) == 6 and np.all(t['best'][planted] == 1) and np.all(t['gap'][planted] == 0) and not np.any(t['best'] == 2)
    main = best_case('main')
    want = inliers_expect_of(main)
    per_pair = np.bincount(main['hyp_pair'], minlength=10)
    assert per_pair.tolist() == [0, 1, 2, 127, 128, 129, 300, 300, 300, 300]
    won = {int(main['hyp_pair'][h]): int(h) for h in want['best_hypotheses']}
    assert 1 in won and 2 not in won and 0 not in won
    for p, apart in zip((6, 7, 8, 9), (1, 127, 128, 129)):
        ids = np.flatnonzero(main['hyp_pair'] == p)
        assert won[p] == ids[5] and want['n_inliers'][ids[5 + apart]] == 8 and bits(want['dists_sum'][ids[5]]) == bits(want['dists_sum'][ids[5 + apart]])
    assert inliers_expect_of(best_case('n_min0'))['best_hypotheses'].tolist() == [1]
    for name in ('zero_unique', 'zero_tied'):
        assert inliers_expect_of(best_case(name))['best_hypotheses'].tolist() == [1]
        assert inliers_expect_of(best_case(name), skip0=False)['best_hypotheses'].tolist() == [0, 1]


def _expected(kinds):
    """what the GPU tests expect, recomputed with whatever ransac_ref holds right now"""
    out = {}
    if 'hyp' in kinds:
        for name in E().HYP_CASES:
            t = rr.ref_hypotheses(*(hyp_case(name)[k] for k in ('poses', 'cand_mesh', 'pts', 'sym', 'n_sym', 'seeds')))
            out['hyp_' + name] = (np.round(t['rows'], 6), t['best'])        # a moved row entry, not a last bit
    if 'walk' in kinds:
        for signed in (False, True):
            out[f'walk_{signed}'] = inliers_expect_of(walk_case(signed))
    if 'best' in kinds:
        for name in E().BEST_CASES:
            out['best_' + name] = inliers_expect_of(best_case(name))
    return out


def _same(a, b):
    if isinstance(a, dict):
        return all(_same(a[k], b[k]) for k in a)
    if isinstance(a, tuple):
        return all(_same(x, y) for x, y in zip(a, b))
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=np.asarray(a).dtype.kind == 'f')


def _pow2(S):
    G = 1
    while G < S:
        G <<= 1
    return G


def _rank_low5(c):
    return np.unique(np.asarray(c), return_inverse=True)[1].reshape(-1) & 31


MUTATIONS = {
    'ties sorted in descending list order': ('walk', 'sort_order', lambda d: np.lexsort((-np.arange(len(d)), np.asarray(d, F32)))),
    '< for <= at the threshold': ('walk', 'inliers', lambda d, thr: np.asarray(d, F32) < F32(thr)),
    'last minimum wins': ('hyp', 'first_min', lambda v, axis=-1: np.asarray(v).shape[axis] - 1 - np.argmin(np.flip(v, axis), axis=axis)),
    'rank word index forced to 0': ('walk', 'used_ids', _rank_low5),
    'an idle lane\'s symmetry admitted': ('hyp', 'lanes', _pow2),
    'n_sym ignored': ('hyp', 'n_real', lambda n_sym, S: int(S)),
    'highest id wins ties': ('best', 'beats', lambda n, s, bn, bs: n > bn or (n == bn and s <= bs)),
    '> for >= at n_min_inliers': ('best', 'reaches', lambda n, n_min: n > n_min),
}


@pytest.mark.parametrize('mistake', list(MUTATIONS))
def test_cases_discriminate(mistake, monkeypatch):
    """Each plausible kernel mistake, made in the twin, changes what at least one case expects: the cases would notice it."""
    kind, name, fn = MUTATIONS[mistake]
    want = _expected({kind})
    monkeypatch.setattr(rr, name, fn)
    got = _expected({kind})
    changed = [k for k in want if not _same(want[k], got[k])]
    print(f'  {mistake}: changes {changed}')
    assert changed


def test_plan_with_an_empty_pair():
    """A view pair without tentative matches, in the middle and in last position: the rank table is built (it used to raise
    IndexError on the last one) and the other pairs' ranks are unchanged.  No GPU, but _Plan asks the built library for its limit
    (cosy_ransac_max_tmatches), as the tests of test_multiview_matching_host.py do: build the library first."""
    import torch
    from cosypose_amd.multiview_matching import TentativeMatches, _Plan, _compact_tmatches
    full = _Plan(TentativeMatches([0, 0], [1, 3], [0, 3, 5], [4, 4, 9, 7, 8], [5, 6, 5, 2, 2], [0, 1, 0]), torch.device('cpu'))
    gaps = _Plan(TentativeMatches([0, 0, 0, 0], [1, 2, 3, 4], [0, 3, 3, 5, 5], [4, 4, 9, 7, 8], [5, 6, 5, 2, 2], [0, 2, 0, 3, 1]), torch.device('cpu'))
    assert torch.equal(full.tm, gaps.tm) and full.tm[:, 2:].tolist() == [[0, 0], [0, 1], [1, 0], [0, 0], [1, 0]]
    assert gaps.pair_hyp_off.tolist() == [0, 2, 3, 4, 5] and gaps.max_tm == 3
    tm = _compact_tmatches(dict(hypothesis_id=[0, 0, 1, 1], cand1=[4, 9, 4, 9], cand2=[5, 5, 5, 5]), [0, 0, 5], [1, 1, 6])
    assert tm.pair_sizes.tolist() == [2, 0] and _Plan(tm, torch.device('cpu')).tm[:, 2:].tolist() == [[0, 0], [1, 0]]


# ---------------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------------
def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def gpu_scene(c):
    """_Scene of a case's float32 tables"""
    import pandas as pd
    from cosypose_amd.mesh_db import BatchedMeshes
    from cosypose_amd.multiview_matching import _Scene
    from cosypose_amd.tensor_collection import PandasTensorCollection
    labels = np.array([f'obj_{i:06d}' for i in range(1, len(c['n_sym']) + 1)])
    mesh_db = BatchedMeshes({l: dict(label=l, n_sym=int(c['n_sym'][i])) for i, l in enumerate(labels)}, labels, dev(c['pts']), dev(c['sym']))
    cand = PandasTensorCollection(pd.DataFrame(dict(view_id=0, label=labels[c['cand_mesh']], score=1.0)), poses=dev(c['poses']))
    return _Scene(cand, mesh_db)


def seeds_dict(table):
    table = np.asarray(table, np.int32).reshape(-1, 4)
    return dict(view1=np.zeros(len(table), np.int32), view2=np.ones(len(table), np.int32), match1_cand1=table[:, 0], match1_cand2=table[:, 1],
                match2_cand1=table[:, 2], match2_cand2=table[:, 3])


def run_hypotheses(scene, table):
    from cosypose_amd.multiview_matching import _hypotheses
    out = _hypotheses(scene, seeds_dict(table), with_sym_dists=True)
    return {k: v.cpu().numpy() for k, v in out.items()}


def own_row_decisions(rows):
    """best_sym and gap as the kernel must derive them from its OWN float32 row: first argmin; second smallest - smallest (float32)"""
    best = rows.argmin(1)
    two = np.sort(rows, axis=1)[:, :2] if rows.shape[1] > 1 else np.concatenate([rows, np.full_like(rows, np.inf)], 1)
    with np.errstate(invalid='ignore'):
        return best, (two[:, 1] - two[:, 0]).astype(F32)


@gpu
@pytest.mark.parametrize('name', ['S1_H1', 'S1_H257', 'S3', 'S5', 'S33', 'S64_H3', 'S64_H4', 'S64_H5', 'tie'])
def test_hypotheses(name):
    """cosy_ransac_hypotheses, EVERY seed: the distance row against the twin under the admissible-symmetry rule (ROW_TOL), inf in the
    same places; best_sym = the first argmin of the kernel's own row and gap = its float32 runner-up difference, exactly; TC1C2
    against the float64 product TC1Oa S_k inv(TC2Ob) for the returned k (TC_TOL); EVERY seed alone gives the bits it gives in the batch.
    'tie' (rows 1 and 2 of the tables are the same bits): index 1 wins, never 2, with gap == 0 where they are the minimum.
    Measured on an MI355X, worst over the cases: rows 3.21e-7 (bound ROW_TOL = 9e-7), TC1C2 2.03e-7 (TC_TOL = 6e-7); per case in
    DESIGN.md section 11."""
    c, t = hyp_case(name), hyp_expect(name)
    share, total = single_admissible_share()
    scene = gpu_scene(c)
    out = run_hypotheses(scene, c['seeds'])
    rows, H = out['sym_dists'], len(c['seeds'])
    err, single = judged(np.where(t['finite'], rows, 0.0), t['dist0'], t['adm'])
    a, b = c['seeds'][:, 0], c['seeds'][:, 1]
    k = out['best_sym']
    w = lambda x: x.astype(np.float64)
    built = w(c['poses'][a]) @ w(c['sym'][c['cand_mesh'][a], np.clip(k, 0, None)]) @ rr.invert_T(w(c['poses'][b]))
    best, gap = own_row_decisions(rows)
    figs = dict(seeds=H, row_err=float(err[t['finite']].max()), single_admissible=f'{int(single[t["finite"]].sum())} / {int(t["finite"].sum())}',
                TC1C2_err=float(np.abs(out['TC1C2'] - built).max()), best_differs_from_twin=int((k != t['best']).sum()),
                gap_zero=int((out['gap'] == 0).sum()), single_admissible_share_all_cases=share)
    print(f'FIGURE hypotheses {name}', figs)
    assert share >= 0.95, (share, total)
    assert np.array_equal(np.isfinite(rows), t['finite']) and np.all(rows[~t['finite']] == np.inf)
    assert figs['row_err'] < ROW_TOL
    assert np.array_equal(k, best)
    assert np.array_equal(bits(out['gap']), bits(gap))
    assert figs['TC1C2_err'] < TC_TOL
    if name == 'tie':
        assert np.all(k[c['planted']] == 1) and np.all(out['gap'][c['planted']] == 0) and not np.any(k == 2)
        assert np.array_equal(bits(rows[:, 1]), bits(rows[:, 2]))
    for h in range(H):                                  # EVERY seed alone: each workgroup position, each same-pair seed
        one = run_hypotheses(scene, c['seeds'][h:h + 1])
        assert all(np.array_equal(one[key].view(np.uint32), out[key][h:h + 1].view(np.uint32)) for key in one), f'seed {h} alone differs'


@gpu
def test_hypotheses_invalid_seeds():
    """Through the raw ABI (the Python layer refuses such ids first): seeds naming candidate -1 or n_cand, or a candidate whose
    cand_mesh row is outside the table (as match 1 or match 2), give best_sym = -1, gap = inf, a zero TC1C2 and leave their
    pre-filled sym_dists row untouched; every other seed gives the bits of a launch without the invalid ones."""
    import torch
    from cosypose_amd._lib import lib, check, ptr, stream
    c = dict(hyp_case('S5'))
    n_cand, n_mesh = len(c['poses']), len(c['n_sym'])
    c['poses'] = np.concatenate([c['poses'], c['poses'][:2]])
    c['cand_mesh'] = np.concatenate([c['cand_mesh'], [0, 0]]).astype(np.int32)
    scene = gpu_scene(c)
    scene.cand_mesh = dev(np.concatenate([c['cand_mesh'][:n_cand], [n_mesh, -1]]).astype(np.int32))      # candidates X = n_cand, Y = n_cand + 1
    X, Y, past = n_cand, n_cand + 1, n_cand + 2
    valid = c['seeds']
    bad = np.array([[-1, 1, 2, 3], [0, past, 2, 3], [0, 1, X, 3], [Y, 1, 2, 3], [0, 1, 2, -1], [0, 1, past, 3], [X, 1, 2, 3]], np.int32)
    where = np.array([0, 1, 5, 30, 31, len(valid) + 5, len(valid) + 6])          # positions of the invalid seeds in the mixed table
    mixed = np.zeros((len(valid) + len(bad), 4), np.int32)
    is_bad = np.zeros(len(mixed), bool)
    is_bad[where] = True
    mixed[is_bad], mixed[~is_bad] = bad, valid

    def launch(table):
        H, S = len(table), scene.S
        seeds = dev(table)
        out = dict(TC1C2=torch.full((H, 4, 4), 7.5, device='cuda'), best_sym=torch.full((H,), 99, dtype=torch.int32, device='cuda'),
                   gap=torch.full((H,), 7.5, device='cuda'), sym_dists=torch.full((H, S), 7.5, device='cuda'))
        check(lib().cosy_ransac_hypotheses(*scene.args(True), ptr(seeds), H, ptr(out['TC1C2']), ptr(out['best_sym']), ptr(out['gap']),
                                           ptr(out['sym_dists']), stream()))
        return {k: v.cpu().numpy() for k, v in out.items()}
    got, base = launch(mixed), launch(valid)
    print('FIGURE invalid seeds', dict(seeds=len(mixed), invalid=int(is_bad.sum()), best_sym=got['best_sym'][is_bad].tolist()))
    assert np.all(got['best_sym'][is_bad] == -1) and np.all(got['gap'][is_bad] == np.inf)
    assert np.all(got['TC1C2'][is_bad] == 0) and np.all(got['sym_dists'][is_bad] == 7.5)
    assert all(np.array_equal(got[k][~is_bad].view(np.uint32), base[k].view(np.uint32)) for k in got)
    assert np.all(base['best_sym'] >= 0) and np.all(base['sym_dists'] != 7.5)


def tmatches_of(pr):
    from cosypose_amd.multiview_matching import TentativeMatches
    return TentativeMatches(pr['pair_view1'], pr['pair_view2'], pr['pair_off'], pr['pair_c1'], pr['pair_c2'], pr['hyp_pair'])


def run_given(pr, skip0=True, n_min=None):
    """_score + _best on the case's distance table -> the inlier dict + n_inliers / dists_sum of EVERY hypothesis"""
    import torch
    from cosypose_amd.multiview_matching import _Plan, _score, _best
    plan = _Plan(tmatches_of(pr), torch.device('cuda'))
    d = dev(pr['dists'])
    n, s, _ = _score(None, plan, None, pr['thr'], dists_in=d)
    out = _best(None, plan, None, n, s, pr['thr'], pr['n_min'] if n_min is None else n_min, skip0, dists_in=d)
    return out, n.cpu().numpy(), s.cpu().numpy()


def assert_inliers_equal(out, n, s, want):
    assert np.array_equal(n, want['n_inliers'])
    assert np.array_equal(bits(s), bits(want['dists_sum'])), 'dists_sum is not the reference\'s float32 sum in walk order'
    assert np.array_equal(out['best_hypotheses'], want['best_hypotheses'])
    assert np.array_equal(out['inlier_matches_cand1'], want['inlier_matches_cand1']) and np.array_equal(out['inlier_matches_cand2'], want['inlier_matches_cand2'])
    assert np.array_equal(out['n_inliers'], want['n_inliers'][want['best_hypotheses']])
    assert np.array_equal(bits(out['dists_sum']), bits(want['dists_sum'][want['best_hypotheses']]))


@gpu
@pytest.mark.parametrize('signed', [False, True], ids=['plain', 'signed'])
def test_score_and_walk_on_given_distances(signed):
    """One launch over view pairs whose lists have 1, 2, 127, 128, 129, 257, 1000 and 4096 matches (per-pair sort sizes 128 .. 4096 under
    one LDS size), three hypotheses each.  Distances are drawn from +0, three values below the threshold, the threshold, the next
    float32 above it, +inf and NaN ('signed': also -0, -0.005 and -1, which the reference's `<` sorts first and ties -0 with +0 by
    position), so exact ties are the rule; the candidates repeat, so the walk skips dozens of conflicting inliers and reaches the
    second and later words of both `used` sets (asserted on the CPU).  n_inliers, dists_sum (bits), best_hypotheses and both match
    lists equal the twin's."""
    pr, want = walk_case(signed), walk_expect(signed)
    out, n, s = run_given(pr)
    per_len = {L: (int(want['n_inliers'][pr['hyp_pair'] == p].max()), int(want['skipped'][pr['hyp_pair'] == p].max())) for p, L in enumerate(E().LENGTHS)}
    print(f'FIGURE given distances {"signed" if signed else "plain"}', dict(inliers_skipped_by_length=per_len, n_differ=int((n != want['n_inliers']).sum()),
                                                                         sum_bits_differ=int((bits(s) != bits(want['dists_sum'])).sum()),
                                                                         winners=out['best_hypotheses'].tolist()))
    assert_inliers_equal(out, n, s, want)


@gpu
@pytest.mark.parametrize('name', ['main', 'n_min0', 'zero_unique', 'zero_tied'])
def test_best_on_crafted_tables(name):
    """Best hypothesis per view pair.  'main': 0, 1, 2, 127, 128, 129 and 300 hypotheses per pair with ids dealt round-robin; the unique
    best row planted twice, 1 / 127 / 128 / 129 positions apart (same thread and different threads of the strided loop): the lower
    id wins; n_inliers == n_min_inliers wins, n_min_inliers - 1 does not.  'n_min0': an inlier-free hypothesis wins at n_min_inliers
    = 0.  'zero_*': hypothesis 0 as the unique best / tied with a later copy: the pair is dropped, and reported with
    skip_hypothesis_0=False."""
    pr = best_case(name)
    want = inliers_expect_of(pr)
    out, n, s = run_given(pr)
    print(f'FIGURE best {name}', dict(hypotheses=len(pr['hyp_pair']), winners=out['best_hypotheses'].tolist(), want=want['best_hypotheses'].tolist()))
    assert_inliers_equal(out, n, s, want)
    with0, n0, s0 = run_given(pr, skip0=False)
    assert_inliers_equal(with0, n0, s0, inliers_expect_of(pr, skip0=False))
    if name.startswith('zero'):
        assert out['best_hypotheses'].tolist() == [1] and with0['best_hypotheses'].tolist() == [0, 1]
    if name == 'main':                   # one lower: the two hypotheses of pair 2 (2 inliers each, different sums) now compete
        low, nl, sl = run_given(pr, n_min=2)
        assert_inliers_equal(low, nl, sl, inliers_expect_of(pr, n_min=2))
        assert len(low['best_hypotheses']) == len(out['best_hypotheses']) + 1


def run_computed(pr, scene=None):
    import torch
    from cosypose_amd.multiview_matching import _Plan, _score, _best
    scene = scene or gpu_scene(pr)
    plan = _Plan(tmatches_of(pr), torch.device('cuda'), scene.n_cand)
    TC = dev(pr['TC1C2'])
    n, s, table = _score(scene, plan, TC, pr['thr'], with_dists=True)
    n2, s2, _ = _score(scene, plan, TC, pr['thr'])
    assert torch.equal(n, n2) and torch.equal(s.view(torch.int32), s2.view(torch.int32)), 'the launch without a table gives other bits'
    out = _best(scene, plan, TC, n, s, pr['thr'], pr['n_min'])
    given = _best(None, plan, None, n, s, pr['thr'], pr['n_min'], dists_in=table)
    assert all(np.array_equal(out[k], given[k]) for k in out), '_best on its own distances and on the table differ'
    return out, n.cpu().numpy(), s.cpu().numpy(), table.cpu().numpy()


@gpu
@pytest.mark.parametrize('n_objects,n_views', [(30, 3), (60, 2)])
def test_score_on_computed_distances(n_objects, n_views):
    """make_ba_scene scenes (8 corners) with doubled candidates: lists of hundreds of matches (cut to 257 / 129 / 128 / 127 / 1000 for some
    pairs), twelve hypotheses per pair.  1. EVERY distance of the table against the twin under the admissible-symmetry rule
    (SCORE_TOL).  2. n_inliers, dists_sum (bits), the winners and their matches EXACTLY equal walk / best_per_pair applied to the
    kernel's own table -- decisions are not judged against float64 (6-17 % of these hypotheses have a distance within 1e-5 of a
    decision).  The production launch without a table, and _best without dists_in, give the same bits.
    Measured on an MI355X: 1.13e-7 (30 objects, 3 views: 13,488 scorings) / 1.37e-7 (60, 2: 28,140); bound SCORE_TOL = 4e-7."""
    pr = score_scene(n_objects, n_views)
    out, n, s, table = run_computed(pr)
    worst, singles, total = 0.0, 0, 0
    for h, sl, dsl, d, dist, cost, L in score_expect(pr):
        err, single = judged(table[dsl], dist, admissible(dist, cost, L, pr['pts'].shape[1]))
        worst = max(worst, float(err.max())); singles += int(single.sum()); total += len(err)
    want = rr.find_inliers(pr['hyp_pair'], pr['pair_off'], pr['pair_c1'], pr['pair_c2'], table, pr['thr'], pr['n_min'])
    sizes = np.diff(pr['pair_off'])
    print(f'FIGURE computed distances {n_objects} x {n_views}', dict(lists=sizes.tolist(), hypotheses=len(n), scorings=total, dist_err=worst,
                                                                     single_admissible=f'{singles} / {total}', median_inliers=float(np.median(want['n_inliers'])),
                                                                     median_skipped=float(np.median(want['skipped'])), winners=out['best_hypotheses'].tolist()))
    assert worst < SCORE_TOL
    assert np.median(want['skipped']) >= 5 and sizes.max() > 256
    assert_inliers_equal(out, n, s, want)


@gpu
def test_nan_pose_only_removes_its_own_matches():
    """A candidate with a NaN pose: its matches are no inliers, and every hypothesis gets the bits of a run in which that candidate's
    matches are taken off the lists."""
    pr = dict(score_scene(30, 3))
    X = int(pr['pair_c1'][0])
    poisoned = dict(pr, poses=pr['poses'].copy())
    poisoned['poses'][X] = np.nan
    keep = (pr['pair_c1'] != X) & (pr['pair_c2'] != X)
    pair_of = np.repeat(np.arange(len(pr['pair_off']) - 1), np.diff(pr['pair_off']))
    cut = dict(pr, pair_c1=pr['pair_c1'][keep], pair_c2=pr['pair_c2'][keep],
               pair_off=np.concatenate([[0], np.cumsum(np.bincount(pair_of[keep], minlength=len(pr['pair_off']) - 1))]).astype(np.int64))
    got, n, s, table = run_computed(poisoned)
    want, wn, ws, _ = run_computed(cut)
    print('FIGURE NaN pose', dict(candidate=X, matches_removed=int((~keep).sum()), nan_distances=int(np.isnan(table).sum()), winners=got['best_hypotheses'].tolist()))
    assert int(np.isnan(table).sum()) == int((~keep[np.concatenate([np.arange(sl.start, sl.stop) for _, sl, _ in E().hyp_rows(pr)])]).sum()) > 0
    assert np.array_equal(n, wn) and np.array_equal(bits(s), bits(ws))
    assert all(np.array_equal(got[k], want[k]) for k in got)


@gpu
def test_empty_last_pair():
    """find_ransac_inliers with an expanded list whose LAST hypothesis (of the last view pair) lists nothing: no winner for that pair,
    the other pairs as without it."""
    from cosypose_amd.multiview_matching import find_ransac_inliers
    pr = best_case('zero_unique')
    rows = E().hyp_rows(pr)
    hyp = np.concatenate([np.full(sl.stop - sl.start, h, np.int32) for h, sl, _ in rows])
    c1, c2 = np.concatenate([pr['pair_c1'][sl] for _, sl, _ in rows]), np.concatenate([pr['pair_c2'][sl] for _, sl, _ in rows])
    v1, v2 = pr['pair_view1'][pr['hyp_pair']], pr['pair_view2'][pr['hyp_pair']]
    base = find_ransac_inliers(v1, v2, hyp, c1, c2, pr['dists'], pr['thr'], pr['n_min'])
    more = find_ransac_inliers(np.append(v1, 9), np.append(v2, 10), hyp, c1, c2, pr['dists'], pr['thr'], pr['n_min'])
    print('FIGURE empty last pair', dict(winners=more['best_hypotheses'].tolist()))
    assert base['best_hypotheses'].tolist() == [1] and all(np.array_equal(base[k], more[k]) for k in base)
    zero = find_ransac_inliers(np.append(v1, 9), np.append(v2, 10), hyp, c1, c2, pr['dists'], pr['thr'], 0)
    assert zero['best_hypotheses'].tolist() == [1, 4] and len(zero['inlier_matches_cand1']) == 4       # the empty hypothesis wins its pair at n_min_inliers = 0
