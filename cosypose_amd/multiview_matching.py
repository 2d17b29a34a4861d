"""Multi-view candidate matching (CosyPose stage 2), same surface as the reference's cosypose/multiview/ransac.py:19-199 and the two
functions of csrc/cosypose_cext.cpp it calls (make_ransac_infos :36-105, find_ransac_inliers :107-216).

Per-view candidates (view_id, label, score, pose TCO) go in; out come the candidates that were matched across views with an `obj_id`
column, one relative camera pose per ordered view pair (`pairs_TC1C2`) and the per-object summary -- the inputs of
bundle_adjustment.MultiviewRefinement.

The reference expands every (hypothesis, tentative match) pair on the host, computes one 4x4 product and one symmetric distance per
pair in batches, copies all distances to the host and finds the inliers in C++.  Here the tentative matches are stored ONCE per
ordered view pair and three launches of libcosyhip.so (kernels_ransac.hip) do the rest: hypotheses, score + inliers fused (the
distances never reach memory), best hypothesis per view pair.  What is read back is one id and one match list per view pair.
float32 throughout, as the reference on its GPU path; inputs of another dtype or layout are narrowed once.

Host work: the tentative-match and seed tables (numpy), the connected components and the pandas frames of the outputs.
"""
import time
from collections.abc import Mapping

import numpy as np
import pandas as pd
import torch

from . import tensor_collection as tc
from ._lib import lib, check, ptr, stream, require_device
from .bundle_adjustment import make_obj_infos, _strong_components, invert_T      # noqa: F401  (make_obj_infos: part of this surface)

SEED_KEYS = ('view1', 'view2', 'match1_cand1', 'match1_cand2', 'match2_cand1', 'match2_cand2')


def max_tmatches():
    """The largest number of tentative matches one ordered view pair may have (the LDS sort of kernels_ransac.hip): 4096."""
    return int(lib().cosy_ransac_max_tmatches())


class TentativeMatches(Mapping):
    """The reference's `tmatches` dict (hypothesis_id, cand1, cand2: every hypothesis paired with every tentative match of its view
    pair) without the expansion: the matches are kept per ordered view pair (`pair_view1`, `pair_view2`, `pair_off`, `pair_cand1`,
    `pair_cand2`) with `hyp_pair` naming each hypothesis's pair.  The three reference keys are expanded on first access."""

    def __init__(self, pair_view1, pair_view2, pair_off, pair_cand1, pair_cand2, hyp_pair):
        self.pair_view1, self.pair_view2 = np.asarray(pair_view1, np.int32), np.asarray(pair_view2, np.int32)
        self.pair_off = np.asarray(pair_off, np.int64)
        self.pair_cand1, self.pair_cand2 = np.asarray(pair_cand1, np.int32), np.asarray(pair_cand2, np.int32)
        self.hyp_pair = np.asarray(hyp_pair, np.int32)
        self._expanded = None

    @property
    def pair_sizes(self):
        return np.diff(self.pair_off)

    def hyp_offsets(self):
        """(H + 1) int64: where each hypothesis's matches start in the expanded list"""
        return np.concatenate([[0], np.cumsum(self.pair_sizes[self.hyp_pair])]).astype(np.int64)

    def _expand(self):
        if self._expanded is None:
            n = self.pair_sizes[self.hyp_pair]
            off = self.hyp_offsets()
            hyp = np.repeat(np.arange(len(n), dtype=np.int32), n)
            rows = np.arange(off[-1], dtype=np.int64) - np.repeat(off[:-1], n) + np.repeat(self.pair_off[self.hyp_pair], n)
            self._expanded = dict(hypothesis_id=hyp, cand1=self.pair_cand1[rows], cand2=self.pair_cand2[rows])
        return self._expanded

    def __getitem__(self, key):
        return self._expand()[key]

    def __iter__(self):
        return iter(('hypothesis_id', 'cand1', 'cand2'))

    def __len__(self):
        return 3


def _tentative_matches(view_ids, labels):
    """Candidates n, m of different views and the same label, grouped by ordered view pair in ascending (view1, view2), within a
    pair n-major / m-minor (cosypose_cext.cpp:41-52)."""
    view_ids = np.asarray(view_ids)
    _, lab = np.unique(np.asarray(labels), return_inverse=True)
    n, m = np.nonzero((lab[:, None] == lab[None, :]) & (view_ids[:, None] != view_ids[None, :]))
    order = np.lexsort((view_ids[m], view_ids[n]))           # stable: keeps (n, m) order within a pair
    n, m = n[order], m[order]
    v1, v2 = view_ids[n], view_ids[m]
    first = np.flatnonzero(np.concatenate([[True], (v1[1:] != v1[:-1]) | (v2[1:] != v2[:-1])])) if len(n) else np.zeros(0, np.int64)
    return v1[first], v2[first], np.concatenate([first, [len(n)]]), n, m


def make_ransac_infos(view_ids, labels, n_ransac_iter=100, seed=0):
    """-> (seeds, tmatches) with the reference's keys (cosypose_cext.cpp:36-105).  seeds: view1, view2, match1_cand1, match1_cand2,
    match2_cand1, match2_cand2 (int32), per ordered view pair min(n_ransac_iter, n_tm (n_tm - 1)) pairs of two DIFFERENT tentative
    matches, drawn as the reference draws them: match 1 runs over one random permutation of the pair's matches, match 2 over another.
    tmatches: a TentativeMatches (hypothesis_id, cand1, cand2).

    The reference permutes with std::shuffle(std::default_random_engine(seed)), whose sequence belongs to libstdc++; this function
    uses numpy's RandomState(seed) / RandomState(seed + 1) and does NOT reproduce that sequence.  What holds as in the reference: no
    seed twice within a view pair, and wherever n_tm (n_tm - 1) <= n_ransac_iter every ordered pair of different matches is drawn."""
    pv1, pv2, pair_off, c1, c2 = _tentative_matches(view_ids, labels)
    cols = {k: [] for k in SEED_KEYS}
    hyp_pair = []
    rng1, rng2 = np.random.RandomState(seed), np.random.RandomState(seed + 1)     # seeded once: seeding costs more than a pair's draw
    for p in range(len(pv1)):
        n_tm = int(pair_off[p + 1] - pair_off[p])
        n_seeds = min(int(n_ransac_iter), n_tm * (n_tm - 1))
        if n_seeds <= 0:
            continue
        perm1, perm2 = rng1.permutation(n_tm), rng2.permutation(n_tm)
        rows = -(-n_seeds // (n_tm - 1))                        # match-1 values needed
        m1 = np.repeat(perm1[:rows], n_tm)
        m2 = np.tile(perm2, rows)
        keep = np.flatnonzero(m1 != m2)[:n_seeds]
        m1, m2 = m1[keep] + pair_off[p], m2[keep] + pair_off[p]
        cols['view1'].append(np.full(n_seeds, pv1[p])); cols['view2'].append(np.full(n_seeds, pv2[p]))
        cols['match1_cand1'].append(c1[m1]); cols['match1_cand2'].append(c2[m1])
        cols['match2_cand1'].append(c1[m2]); cols['match2_cand2'].append(c2[m2])
        hyp_pair.append(np.full(n_seeds, p))
    cat = lambda l: np.concatenate(l).astype(np.int32) if l else np.zeros(0, np.int32)
    seeds = {k: cat(v) for k, v in cols.items()}
    return seeds, TentativeMatches(pv1, pv2, pair_off, c1, c2, cat(hyp_pair))


def _compact_tmatches(tmatches, view1, view2):
    """A TentativeMatches from the reference's expanded dict: the matches of a view pair are taken from its first hypothesis; every
    other hypothesis of the pair must have as many."""
    if isinstance(tmatches, TentativeMatches):
        return tmatches
    hyp = np.asarray(tmatches['hypothesis_id']).astype(np.int64)
    c1, c2 = np.asarray(tmatches['cand1']).astype(np.int32), np.asarray(tmatches['cand2']).astype(np.int32)
    view1, view2 = np.asarray(view1), np.asarray(view2)
    H = len(view1)
    if len(hyp) and (np.any(np.diff(hyp) < 0) or hyp[0] < 0 or hyp[-1] >= H):
        raise ValueError('tmatches: hypothesis_id must be ascending and within the seeds')
    counts = np.bincount(hyp, minlength=H)
    starts = np.concatenate([[0], np.cumsum(counts)])
    pairs, hyp_pair = np.unique(np.stack([view1, view2], 1), axis=0, return_inverse=True) if H else (np.zeros((0, 2), np.int64), np.zeros(0, np.int64))
    hyp_pair = np.asarray(hyp_pair).reshape(-1)
    first_hyp = np.full(len(pairs), H, np.int64)
    np.minimum.at(first_hyp, hyp_pair, np.arange(H))
    if np.any(counts != counts[first_hyp][hyp_pair]):
        raise ValueError('tmatches: the hypotheses of a view pair list different numbers of tentative matches')
    sizes = counts[first_hyp]
    pair_off = np.concatenate([[0], np.cumsum(sizes)])
    rows = np.concatenate([np.arange(starts[h], starts[h] + counts[h]) for h in first_hyp]) if len(pairs) else np.zeros(0, np.int64)
    return TentativeMatches(pairs[:, 0], pairs[:, 1], pair_off, c1[rows.astype(np.int64)], c2[rows.astype(np.int64)], hyp_pair)


class _Plan:
    """The id tables of one matching problem on the device (int32 unless said): hyp_pair (H), pair_off (n_pairs + 1), tm (n_tm, 4:
    cand1, cand2, rank of cand1 / of cand2 within the pair), pair_hyp_off (n_pairs + 1), pair_hyps (H), hyp_dist_off (H, int64)."""

    def __init__(self, tm, device, n_cand=None):
        self.tmatches = tm
        self.H, self.n_pairs = len(tm.hyp_pair), len(tm.pair_view1)
        sizes = tm.pair_sizes
        self.max_tm = int(sizes.max()) if len(sizes) else 0
        if self.max_tm > max_tmatches():
            # the C entries answer COSY_ESIZE too; here before anything is uploaded
            check(lib().cosy_ransac_score(None, None, None, None, 0, 0, 0, 0, None, None, 0, None, None, 0, self.max_tm, 0.0, None, None, None, None,
                                          None, None))
        if self.H and (tm.hyp_pair.min() < 0 or tm.hyp_pair.max() >= self.n_pairs):
            raise ValueError('a hypothesis names a view pair that has no tentative matches')
        c1, c2 = tm.pair_cand1, tm.pair_cand2
        if n_cand is not None and len(c1) and (min(c1.min(), c2.min()) < 0 or max(c1.max(), c2.max()) >= n_cand):
            raise ValueError(f'tentative matches name a candidate outside [0, {n_cand})')
        pair_of = np.repeat(np.arange(self.n_pairs, dtype=np.int64), sizes)
        span = int(max(c1.max(), c2.max())) + 1 if len(c1) else 1
        table = np.zeros((len(c1), 4), np.int32)
        table[:, 0], table[:, 1] = c1, c2
        for col, c in ((2, c1), (3, c2)):                       # rank of the candidate among the pair's candidates on that side
            _, rank = np.unique(pair_of * span + c, return_inverse=True)
            rank = np.asarray(rank).reshape(-1)
            first = np.zeros(self.n_pairs, rank.dtype)              # a pair without matches (the last one too) has no rank to reduce
            if len(rank):
                first[sizes > 0] = np.minimum.reduceat(rank, tm.pair_off[:-1][sizes > 0])
            table[:, col] = rank - first[pair_of]
        order = np.argsort(tm.hyp_pair, kind='stable')
        pair_hyp_off = np.concatenate([[0], np.cumsum(np.bincount(tm.hyp_pair, minlength=self.n_pairs))])
        self.hyp_off_host = tm.hyp_offsets()
        self.n_scorings = int(self.hyp_off_host[-1])
        up = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a)).to(dt).to(device)
        self.hyp_pair, self.pair_off, self.tm = up(tm.hyp_pair, torch.int32), up(tm.pair_off, torch.int32), up(table, torch.int32)
        self.pair_hyp_off, self.pair_hyps = up(pair_hyp_off, torch.int32), up(order, torch.int32)
        self.hyp_dist_off = up(self.hyp_off_host[:-1], torch.int64)
        self.device = device


class _Scene:
    """The candidates' poses and the mesh tables as the kernels read them: float32, contiguous, on the device."""

    def __init__(self, candidates, mesh_db):
        poses = candidates.poses
        require_device(poses, mesh_db.points, mesh_db.symmetries)
        dev = poses.device
        self.poses = poses.detach().to(torch.float32).contiguous()
        self.pts = mesh_db.points.detach().to(torch.float32).contiguous()
        self.sym = mesh_db.symmetries.detach().to(torch.float32).contiguous()
        self.cand_mesh = mesh_db.object_ids(list(candidates.infos['label'].values), dev)
        n_sym = np.fromiter((mesh_db.infos[l]['n_sym'] for l in mesh_db.labels), dtype=np.int32, count=len(mesh_db.labels))
        self.n_sym = torch.as_tensor(n_sym).to(dev)
        self.n_cand, self.n_mesh, self.P, self.S = self.poses.shape[0], self.pts.shape[0], self.pts.shape[1], self.sym.shape[1]
        self.device = dev

    def args(self, with_n_sym=False):
        a = [ptr(self.poses), ptr(self.cand_mesh), ptr(self.pts), ptr(self.sym)]
        return a + ([ptr(self.n_sym)] if with_n_sym else []) + [self.n_cand, self.n_mesh, self.P, self.S]


def _seed_table(seeds, n_cand):
    table = np.stack([np.asarray(seeds[k]).astype(np.int32) for k in SEED_KEYS[2:]], 1) if len(seeds['view1']) else np.zeros((0, 4), np.int32)
    if table.size and (table.min() < 0 or table.max() >= n_cand):
        raise ValueError(f'seeds name a candidate outside [0, {n_cand})')
    return np.ascontiguousarray(table)


def _hypotheses(scene, seeds, with_sym_dists=False):
    """one launch of cosy_ransac_hypotheses -> dict(TC1C2 (H,4,4), best_sym (H) int32, gap (H)[, sym_dists (H,S)])"""
    table = torch.as_tensor(_seed_table(seeds, scene.n_cand)).to(scene.device)
    H, dev = table.shape[0], scene.device
    out = dict(TC1C2=torch.empty(H, 4, 4, device=dev), best_sym=torch.empty(H, dtype=torch.int32, device=dev), gap=torch.empty(H, device=dev))
    if with_sym_dists:
        out['sym_dists'] = torch.empty(H, scene.S, device=dev)
    check(lib().cosy_ransac_hypotheses(*scene.args(True), ptr(table), H, ptr(out['TC1C2']), ptr(out['best_sym']), ptr(out['gap']),
                                       ptr(out.get('sym_dists')), stream()))
    return out


def _score(scene, plan, TC1C2, dist_threshold, dists_in=None, with_dists=False):
    """one launch of cosy_ransac_score -> (n_inliers (H) int32, dists_sum (H), the distance table or None)"""
    dev = plan.device
    n_inliers = torch.empty(plan.H, dtype=torch.int32, device=dev)
    dists_sum = torch.empty(plan.H, device=dev)
    dists = torch.empty(plan.n_scorings, device=dev) if with_dists else None
    scene_args = scene.args() if scene is not None else [None, None, None, None, 0, 0, 0, 0]
    check(lib().cosy_ransac_score(*scene_args, ptr(TC1C2), ptr(plan.hyp_pair), plan.H, ptr(plan.pair_off), ptr(plan.tm), plan.n_pairs, plan.max_tm,
                                  float(dist_threshold), ptr(plan.hyp_dist_off), ptr(dists_in), ptr(dists), ptr(n_inliers), ptr(dists_sum), stream()))
    return n_inliers, dists_sum, dists


def _best(scene, plan, TC1C2, n_inliers, dists_sum, dist_threshold, n_min_inliers, skip_hypothesis_0=True, dists_in=None):
    """one launch of cosy_ransac_best and the read-back -> the reference's `inliers` dict (numpy int32: inlier_matches_cand1,
    inlier_matches_cand2, best_hypotheses) + n_inliers / dists_sum of the winners"""
    dev = plan.device
    best_hyp = torch.empty(plan.n_pairs, dtype=torch.int32, device=dev)
    n_matches = torch.empty(plan.n_pairs, dtype=torch.int32, device=dev)
    match = torch.zeros(2, max(len(plan.tmatches.pair_cand1), 1), dtype=torch.int32, device=dev)
    scene_args = scene.args() if scene is not None else [None, None, None, None, 0, 0, 0, 0]
    check(lib().cosy_ransac_best(*scene_args, ptr(TC1C2), plan.H, ptr(n_inliers), ptr(dists_sum), ptr(plan.pair_hyp_off), ptr(plan.pair_hyps),
                                 ptr(plan.pair_off), ptr(plan.tm), plan.n_pairs, plan.max_tm, float(dist_threshold), int(n_min_inliers),
                                 1 if skip_hypothesis_0 else 0, ptr(plan.hyp_dist_off), ptr(dists_in), ptr(best_hyp), ptr(n_matches), ptr(match[0]),
                                 ptr(match[1]), stream()))
    best_hyp, n_matches, match = best_hyp.cpu().numpy(), n_matches.cpu().numpy(), match.cpu().numpy()
    won = np.flatnonzero(best_hyp >= 0)
    rows = np.concatenate([plan.tmatches.pair_off[p] + np.arange(n_matches[p]) for p in won]).astype(np.int64) if len(won) else np.zeros(0, np.int64)
    best = best_hyp[won].astype(np.int64)
    return dict(inlier_matches_cand1=match[0][rows].astype(np.int32), inlier_matches_cand2=match[1][rows].astype(np.int32),
                best_hypotheses=best_hyp[won].astype(np.int32), n_inliers=n_inliers[best].cpu().numpy() if len(won) else np.zeros(0, np.int32),
                dists_sum=dists_sum[best].cpu().numpy() if len(won) else np.zeros(0, np.float32))


def _empty_inliers():
    z = np.zeros(0, np.int32)
    return dict(inlier_matches_cand1=z, inlier_matches_cand2=z.copy(), best_hypotheses=z.copy(), n_inliers=z.copy(), dists_sum=np.zeros(0, np.float32))


# ---- the reference's functions ---------------------------------------------------------------------------------------------------
def estimate_camera_poses_batch(candidates, seeds, mesh_db, bsz=1024):
    """TC1C2 (H,4,4) of every seed (reference :19-64).  `bsz` is accepted and unused: nothing per (seed, symmetry) is stored, one
    launch serves any number of seeds."""
    return _hypotheses(_Scene(candidates, mesh_db), seeds)['TC1C2']


def score_tmaches_batch(candidates, tmatches, TC1C2, mesh_db, bsz=4096, seeds=None):
    """The distance of every (hypothesis, tentative match) pair in the reference's order (reference :67-88): the TEST path, which
    writes the table the production path never forms.  `tmatches`: a TentativeMatches, or the reference's expanded dict together
    with `seeds` (for the hypotheses' view pairs).  `bsz` is accepted and unused."""
    if not isinstance(tmatches, TentativeMatches):
        if seeds is None:
            raise ValueError('score_tmaches_batch: an expanded tmatches dict needs `seeds`')
        tmatches = _compact_tmatches(tmatches, seeds['view1'], seeds['view2'])
    scene = _Scene(candidates, mesh_db)
    plan = _Plan(tmatches, scene.device, scene.n_cand)
    if plan.H == 0:
        return torch.empty(0, device=scene.device)
    return _score(scene, plan, _as_TC1C2(TC1C2, plan.H, scene.device), np.inf, with_dists=True)[2]


score_tmatches_batch = score_tmaches_batch


def _as_TC1C2(TC1C2, H, device):
    TC1C2 = torch.as_tensor(TC1C2).detach().to(device).to(torch.float32).contiguous()
    if TC1C2.shape != (H, 4, 4):
        raise ValueError(f'TC1C2 has shape {tuple(TC1C2.shape)}, expected {(H, 4, 4)}')
    return TC1C2


def find_ransac_inliers(seeds_view1, seeds_view2, tmatches_hypothesis_id, tmatches_cand1, tmatches_cand2, dists, dist_threshold, n_min_inliers,
                        skip_hypothesis_0=True, device='cuda'):
    """cosypose_cext.find_ransac_inliers (:107-216) on GIVEN distances (one per expanded tentative match), on the device: -> dict of
    numpy int32 arrays inlier_matches_cand1, inlier_matches_cand2, best_hypotheses (plus n_inliers / dists_sum of the winners).
    skip_hypothesis_0=True keeps the reference's `hypothesis_id > 0` test, under which hypothesis 0 never wins."""
    tm = _compact_tmatches(dict(hypothesis_id=tmatches_hypothesis_id, cand1=tmatches_cand1, cand2=tmatches_cand2), seeds_view1, seeds_view2)
    device = dists.device if isinstance(dists, torch.Tensor) and dists.is_cuda else torch.device(device)
    plan = _Plan(tm, device)
    if plan.H == 0:
        return _empty_inliers()
    dists = torch.as_tensor(dists).detach().to(device).to(torch.float32).contiguous()
    if dists.shape != (plan.n_scorings,):
        raise ValueError(f'dists has shape {tuple(dists.shape)}, expected {(plan.n_scorings,)}')
    n_inliers, dists_sum, _ = _score(None, plan, None, dist_threshold, dists_in=dists)
    return _best(None, plan, None, n_inliers, dists_sum, dist_threshold, n_min_inliers, skip_hypothesis_0, dists_in=dists)


def estimate_camera_poses(candidates, seeds, mesh_db):
    """estimate_camera_poses_batch with what decided it: dict(TC1C2 (H,4,4), best_sym (H) the chosen symmetry of match 1's label, gap
    (H) the runner-up's distance minus the minimum (inf with one symmetry), sym_dists (H,S) every symmetry's distance)."""
    return _hypotheses(_Scene(candidates, mesh_db), seeds, with_sym_dists=True)


def score_hypotheses(candidates, tmatches, TC1C2, mesh_db, dist_threshold=0.02, seeds=None, return_dists=False):
    """(n_inliers (H) int32, dists_sum (H)) of every hypothesis on the device: the fused production launch.  return_dists=True adds
    the distance table of score_tmaches_batch, written by the same launch."""
    if not isinstance(tmatches, TentativeMatches):
        tmatches = _compact_tmatches(tmatches, seeds['view1'], seeds['view2'])
    scene = _Scene(candidates, mesh_db)
    plan = _Plan(tmatches, scene.device, scene.n_cand)
    out = _score(scene, plan, _as_TC1C2(TC1C2, plan.H, scene.device), dist_threshold, with_dists=return_dists)
    return out if return_dists else out[:2]


def scene_level_matching(candidates, inliers):
    """Candidates linked by inlier matches in BOTH directions form an object: strongly connected components of cand1 -> cand2
    (reference :91-116).  Candidates of components with fewer than 2 members are dropped, the others keep their order and get
    `obj_id` 0..n-1, numbered by first appearance (the reference's numbers are scipy's; the partition is the same)."""
    n_cand = len(candidates)
    cand1, cand2 = np.asarray(inliers['inlier_matches_cand1']), np.asarray(inliers['inlier_matches_cand2'])
    comp = _strong_components(n_cand, list(zip(cand1.tolist(), cand2.tolist())))
    keep = np.flatnonzero(np.bincount(comp, minlength=n_cand + 1)[comp] >= 2) if n_cand else np.zeros(0, np.int64)
    infos = candidates.infos.iloc[keep].reset_index(drop=True)
    _, first, inverse = np.unique(comp[keep], return_index=True, return_inverse=True)
    infos['obj_id'] = np.argsort(np.argsort(first))[np.asarray(inverse).reshape(-1)] if len(keep) else np.zeros(0, np.int64)
    ids = torch.as_tensor(keep, dtype=torch.long, device=candidates.poses.device)
    return tc.PandasTensorCollection(infos=infos, poses=torch.index_select(candidates.poses, 0, ids))


def get_best_viewpair_pose_est(TC1C2, seeds, inliers):
    """One row per view pair that has a best hypothesis: view1, view2, TC1C2 (reference :128-134)."""
    best = np.asarray(inliers['best_hypotheses']).astype(np.int64)
    infos = pd.DataFrame(dict(view1=np.asarray(seeds['view1'])[best], view2=np.asarray(seeds['view2'])[best]))
    ids = torch.as_tensor(best, dtype=torch.long, device=TC1C2.device)
    return tc.PandasTensorCollection(infos=infos, TC1C2=torch.index_select(TC1C2, 0, ids))


def multiview_candidate_matching(candidates, mesh_db, model_bsz=1e3, score_bsz=1e5, dist_threshold=0.02, cameras=None, n_ransac_iter=20,
                                 n_min_inliers=3, seeds=None, skip_hypothesis_0=True):
    """Reference :137-199.  candidates: PandasTensorCollection with infos view_id, label, score and poses (n,4,4) on the device;
    mesh_db: BatchedMeshes of the points the distance is taken over (the reference uses the 8 bounding-box corners).  With
    `cameras` (infos view_id, TWC) the camera poses are known: one hypothesis per view pair, TC1C2 = inv(TWC1) TWC2.
    -> dict(filtered_candidates, scene_infos, pairs_TC1C2, time_models, time_score, time_misc) + `inliers`, the inlier dict.

    seeds: the RANSAC seeds to use instead of make_ransac_infos(view_id, label, n_ransac_iter, 0)'s (a reproducible run, or another
    sampler); the tentative matches always follow from the candidates.  model_bsz / score_bsz are accepted and unused (nothing is
    stored per scoring, so there is nothing to batch).  skip_hypothesis_0=True reproduces the reference, whose test
    `best_hypothesis.hypothesis_id > 0` never lets hypothesis 0 win: with known camera poses the first view pair is always
    dropped.  A scene without tentative matches, without a view pair reaching n_min_inliers, or with one view gives empty outputs."""
    times = dict(models=0.0, score=0.0, misc=0.0)

    def timed(name, t0):
        if candidates.poses.is_cuda:
            torch.cuda.synchronize()
        times[name] += time.time() - t0

    known_poses = cameras is not None
    if known_poses:
        n_ransac_iter = 1
    t0 = time.time()
    candidates.infos['cand_id'] = np.arange(len(candidates))
    timed('misc', t0)

    t0 = time.time()
    view_ids, labels = candidates.infos['view_id'].values, candidates.infos['label'].values
    if seeds is None:
        seeds, tmatches = make_ransac_infos(view_ids, labels, n_ransac_iter, 0)
    else:
        seeds = {k: np.asarray(seeds[k]).astype(np.int32) for k in SEED_KEYS}
        pv1, pv2, pair_off, c1, c2 = _tentative_matches(view_ids, labels)
        pair_index = {(a, b): n for n, (a, b) in enumerate(zip(pv1.tolist(), pv2.tolist()))}
        try:
            hyp_pair = [pair_index[k] for k in zip(seeds['view1'].tolist(), seeds['view2'].tolist())]
        except KeyError as e:
            raise ValueError(f'seeds name the view pair {e.args[0]}, which has no tentative matches') from None
        tmatches = TentativeMatches(pv1, pv2, pair_off, c1, c2, hyp_pair)
    H = len(seeds['view1'])
    scene = plan = TC1C2 = None
    if H:
        scene = _Scene(candidates, mesh_db)
        plan = _Plan(tmatches, scene.device, scene.n_cand)
        if not known_poses:
            TC1C2 = _hypotheses(scene, seeds)['TC1C2']
        else:
            idx = pd.Series(np.arange(len(cameras)), index=cameras.infos['view_id'].values)
            TWC = cameras.TWC.detach().to(scene.device).to(torch.float32)
            TWC1, TWC2 = TWC[idx.loc[seeds['view1']].values], TWC[idx.loc[seeds['view2']].values]
            TC1C2 = (invert_T(TWC1) @ TWC2).contiguous()
    timed('models', t0)

    t0 = time.time()
    if H:
        n_inliers, dists_sum, _ = _score(scene, plan, TC1C2, dist_threshold)
        inliers = _best(scene, plan, TC1C2, n_inliers, dists_sum, dist_threshold, n_min_inliers, skip_hypothesis_0)
    else:
        inliers = _empty_inliers()
        TC1C2 = torch.empty(0, 4, 4, dtype=torch.float32, device=candidates.poses.device)
    timed('score', t0)

    t0 = time.time()
    pairs_TC1C2 = get_best_viewpair_pose_est(TC1C2, seeds, inliers)
    filtered_candidates = scene_level_matching(candidates, inliers)
    scene_infos = make_obj_infos(filtered_candidates)
    timed('misc', t0)
    return dict(filtered_candidates=filtered_candidates, scene_infos=scene_infos, pairs_TC1C2=pairs_TC1C2, time_models=times['models'],
                time_score=times['score'], time_misc=times['misc'], inliers=inliers)
