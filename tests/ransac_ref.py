"""Numpy twins of multi-view candidate matching (cosypose_amd/multiview_matching.py, csrc/kernels_ransac.hip), restated from the
reference's text and held to the reference's own float64 run by tests/test_ransac_kernels.py::test_twin_vs_reference
(tests/golden/reference_golden_ransac_edges.npz).  numpy only: nothing here imports the package or torch.

Every function takes the float32 inputs a kernel is given and widens them to float64; the bookkeeping (inliers, order, sums, best
hypothesis) works on float32 distances, as the reference's C++ does.

Twins
  * ref_fast_distance   cosypose/lib3d/symmetric_distances.py:38-57
  * ref_hypotheses      cosypose/multiview/ransac.py:19-47  (invert_T: lib3d/transform_ops.py:24-32)
  * ref_score           cosypose/multiview/ransac.py:67-88
  * walk, best_per_pair cosypose/csrc/cosypose_cext.cpp:156-210  (sort_indexes: :19-25)

The small functions first_min / n_real / lanes / inliers / sort_order / used_ids / beats / reaches are the single decisions of
these twins; test_cases_discriminate replaces them one at a time with a plausible kernel mistake and requires the expected output
of some case to change.
"""
import numpy as np

F32 = np.float32
U = 2.0 ** -24            # float32 unit roundoff


# ---- the single decisions ----------------------------------------------------------------------------------------------------------
def first_min(values, axis=-1):
    """argmin under strict <: the first minimum stays (torch.argmin symmetric_distances.py:53; scatter_argmin cosypose_cext.cpp:218-246)"""
    return np.argmin(values, axis=axis)


def n_real(n_sym, S):
    """symmetries of a label that expand_ids_for_symmetry lists (ransac.py:35): n_sym of the padded table's S rows"""
    return int(min(max(int(n_sym), 1), S))


def lanes(S):
    """rows of the padded table that symmetric_distance_batched_fast compares (symmetric_distances.py:49): all S, nothing more"""
    return int(S)


def inliers(d32, thr):
    """cosypose_cext.cpp:161: dist <= dist_threshold, both float32 (NaN is none)"""
    with np.errstate(invalid='ignore'):
        return np.asarray(d32, F32) <= F32(thr)


def sort_order(d):
    """cosypose_cext.cpp:19-25: stable_sort of the indices with v[i1] < v[i2] (so -0 ties with +0 and ties keep their order)"""
    return np.argsort(np.asarray(d, F32), kind='stable')


def used_ids(c):
    """what the `matched` sets hold (cosypose_cext.cpp:172-178): the candidate ids themselves"""
    return np.asarray(c)


def beats(n, s, bn, bs):
    """cosypose_cext.cpp:197-199: more inliers, or as many and a strictly smaller sum: the first of equals is kept"""
    return n > bn or (n == bn and s < bs)


def reaches(n, n_min_inliers):
    """cosypose_cext.cpp:196"""
    return n >= n_min_inliers


# ---- distances ---------------------------------------------------------------------------------------------------------------------
def _w(a):
    """float32 inputs widen exactly; float64 intermediates pass through"""
    return np.asarray(a, np.float64)


def invert_T(T):
    """transform_ops.py:24-32: R^T, -R^T t, the last row kept"""
    T = np.asarray(T, np.float64)
    out = T.copy()
    Rt = np.swapaxes(T[..., :3, :3], -1, -2)
    out[..., :3, :3] = Rt
    out[..., :3, 3] = -(Rt @ T[..., :3, 3:4])[..., 0]
    return out


def transform_pts(T, pts):
    """transform_ops.py:7-21: R p + t; T (...,4,4), pts (...,P,3) -> (...,P,3)"""
    return np.einsum('...ij,...pj->...pi', T[..., :3, :3], pts) + T[..., None, :3, 3]


def ref_fast_distance(T1, T2, pts, sym):
    """symmetric_distance_batched_fast (symmetric_distances.py:38-57) per item: T1, T2 (B,4,4), pts (B,P,3), sym (B,S,4,4) the padded
    table of the item's label.  -> (dist (B,S), cost (B,S)): for EVERY symmetry k the mean distance and the mean squared distance
    between T1 S_k p and T2 p.  The function's result is dist[b, first_min(cost[b])]."""
    T1, T2, pts, sym = _w(T1), _w(T2), _w(pts), _w(sym)
    p1 = transform_pts(T1[:, None] @ sym, pts[:, None])                # :49
    p2 = transform_pts(T2, pts)[:, None]                               # :50
    sq = ((p1 - p2) ** 2).sum(-1)                                      # :52  (B,S,P)
    return np.sqrt(sq).mean(-1), sq.mean(-1)                           # :55, :53


def ref_hypotheses(poses, cand_mesh, pts, sym, n_sym, seeds):
    """estimate_camera_poses (ransac.py:19-47).  poses (n_cand,4,4), cand_mesh (n_cand) the table row of each candidate's label, pts
    (n_mesh,P,3), sym (n_mesh,S,4,4) identity-padded, n_sym (n_mesh), seeds (H,4) = match1_cand1 (a), match1_cand2 (b), match2_cand1 (g),
    match2_cand2 (d).  For symmetry s of a's label: T2 = (TC1Oa S_s inv(TC2Ob)) TC2Od (:41), distance = fast distance of TC1Og and T2
    over g's label.  -> dict
      rows  (H,S)    the distance of every s, inf past the label's n_sym
      best  (H)      the first minimum of the row (:44)
      gap   (H)      second smallest - smallest of the row (inf with one symmetry)
      TC1C2 (H,4,4)  TC1Oa S_best inv(TC2Ob) (:45-46)
      dist, cost (H,S,L)  per s the distance / mean squared cost of every symmetry of g's label (what decides rows)"""
    poses, pts_t, sym_t = _w(poses), _w(pts), _w(sym)
    seeds = np.asarray(seeds).reshape(-1, 4)
    H, S, L = len(seeds), sym_t.shape[1], lanes(sym_t.shape[1])
    flat = sym_t.reshape(-1, 4, 4)
    rows = np.full((H, S), np.inf)
    dist, cost = np.full((H, S, L), np.inf), np.full((H, S, L), np.inf)
    best, gap, TC1C2 = np.zeros(H, np.int64), np.full(H, np.inf), np.zeros((H, 4, 4))
    for h, (a, b, g, d) in enumerate(seeds.tolist()):
        m_ab, m_gd = int(cand_mesh[a]), int(cand_mesh[g])
        TObC2 = invert_T(poses[b])                                     # :32
        ns = n_real(n_sym[m_ab], S)
        table = flat[(m_gd * S + np.arange(L)) % len(flat)]            # L == S: the label's own rows
        T2 = (poses[a] @ sym_t[m_ab, :ns] @ TObC2) @ poses[d]          # :41
        dd, cc = ref_fast_distance(np.repeat(poses[g][None], ns, 0), T2, np.repeat(pts_t[m_gd][None], ns, 0), np.repeat(table[None], ns, 0))
        dist[h, :ns], cost[h, :ns] = dd, cc
        rows[h, :ns] = dd[np.arange(ns), first_min(cc, 1)]
        best[h] = first_min(rows[h, :ns].astype(F32))                 # scatter_argmin compares `dists.float()` (symmetric_distances.py:14)
        if ns > 1:
            two = np.sort(rows[h, :ns])[:2]
            gap[h] = two[1] - two[0]
        TC1C2[h] = poses[a] @ sym_t[m_ab, best[h]] @ TObC2             # :45-46
    return dict(rows=rows, best=best, gap=gap, TC1C2=TC1C2, dist=dist, cost=cost)


def ref_score(poses, cand_mesh, pts, sym, TC1C2, c1, c2):
    """score_tmatches (ransac.py:67-88) of ONE hypothesis over the tentative matches (c1, c2) of its view pair: TWOa = TC1Oa, TWOb =
    TC1C2 TC2Ob (:68-69), fast distance over the label of cand1 (:82).  -> (d (n), dist (n,S), cost (n,S)): the function's distance
    and what every symmetry gives."""
    poses = _w(poses)
    c1, c2 = np.asarray(c1), np.asarray(c2)
    m = np.asarray(cand_mesh)[c1]
    dist, cost = ref_fast_distance(poses[c1], _w(TC1C2)[None] @ poses[c2], np.asarray(pts, F32)[m], np.asarray(sym, F32)[m])
    return dist[np.arange(len(c1)), first_min(cost, 1)], dist, cost


# ---- inliers and the best hypothesis: cosypose_cext.cpp:156-210 ---------------------------------------------------------------------
def walk(c1, c2, d32, thr):
    """One hypothesis (cosypose_cext.cpp:156-185): the inliers d <= thr (float32 both) in stable order of `<`, each cand1 and each
    cand2 used once, dists_sum added in float32 in walk order.  -> (n_inliers, float32 dists_sum, [(cand1, cand2)], inliers skipped
    because a candidate was already used)"""
    d32 = np.asarray(d32, F32)
    pos = np.flatnonzero(inliers(d32, thr))
    pos = pos[sort_order(d32[pos])]
    k1, k2 = used_ids(c1), used_ids(c2)
    used1, used2, total, matches, skipped = set(), set(), F32(0), [], 0
    for i in pos.tolist():
        if int(k1[i]) in used1 or int(k2[i]) in used2:
            skipped += 1
            continue
        used1.add(int(k1[i])); used2.add(int(k2[i]))
        total = F32(total + d32[i])
        matches.append((int(c1[i]), int(c2[i])))
    return len(matches), total, matches, skipped


def best_per_pair(hyp_pair, n_pairs, n_inl, dsum, n_min_inliers, skip_hypothesis_0=True):
    """cosypose_cext.cpp:187-210: per view pair, over its hypotheses in ascending id, the one that reaches n_min_inliers and beats the
    best so far (which starts at 0 inliers, sum FLT_MAX); `hypothesis_id > 0` is required of the winner (:203).
    -> [(pair, hypothesis)] in pair order"""
    hyp_pair = np.asarray(hyp_pair)
    out = []
    for p in range(n_pairs):
        best, bn, bs = -1, 0, np.finfo(F32).max
        for h in np.flatnonzero(hyp_pair == p).tolist():
            if reaches(int(n_inl[h]), n_min_inliers) and beats(int(n_inl[h]), F32(dsum[h]), bn, bs):
                best, bn, bs = h, int(n_inl[h]), F32(dsum[h])
        if best > 0 or (best == 0 and not skip_hypothesis_0):
            out.append((p, best))
    return out


def find_inliers(hyp_pair, pair_off, pair_c1, pair_c2, dists, thr, n_min_inliers, skip_hypothesis_0=True):
    """find_ransac_inliers (cosypose_cext.cpp:107-216) on the compact layout: the hypotheses' view pairs, the pairs' match lists and
    one float32 distance per (hypothesis, match) in hypothesis order.  -> dict(n_inliers (H), dists_sum (H) float32, skipped (H),
    best_hypotheses, inlier_matches_cand1, inlier_matches_cand2)"""
    hyp_pair, pair_off = np.asarray(hyp_pair), np.asarray(pair_off)
    H = len(hyp_pair)
    sizes = np.diff(pair_off)[hyp_pair] if H else np.zeros(0, np.int64)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n_inl, dsum, skipped, matches = np.zeros(H, np.int32), np.zeros(H, F32), np.zeros(H, np.int64), []
    for h in range(H):
        sl = slice(pair_off[hyp_pair[h]], pair_off[hyp_pair[h] + 1])
        n_inl[h], dsum[h], m, skipped[h] = walk(pair_c1[sl], pair_c2[sl], dists[off[h]:off[h + 1]], thr)
        matches.append(m)
    winners = best_per_pair(hyp_pair, len(pair_off) - 1, n_inl, dsum, n_min_inliers, skip_hypothesis_0)
    flat = [m for _, h in winners for m in matches[h]]
    return dict(n_inliers=n_inl, dists_sum=dsum, skipped=skipped, best_hypotheses=np.array([h for _, h in winners], np.int32),
                inlier_matches_cand1=np.array([a for a, _ in flat], np.int32), inlier_matches_cand2=np.array([b for _, b in flat], np.int32))
