"""Host half of the multi-view candidate matching (cosypose_amd/multiview_matching.py) against the reference's outputs stored in
tests/golden/reference_golden_ransac.npz (tests/golden/generate_golden_ransac.py).  No GPU: id tables, graph and frame logic only."""
import re

import numpy as np
import pandas as pd
import pytest
import torch

import ransac_case as rc


@pytest.fixture(scope='module')
def g():
    return rc.load()


def labels_of(scene):
    return np.array([f'obj_{i:06d}' for i in range(1, len(scene['n_sym']) + 1)])[scene['cand_label_id']]


@pytest.mark.parametrize('prefix,n_iter', [('a_', 2000), ('b_', 50)])
def test_make_ransac_infos_structure(g, prefix, n_iter):
    """Tentative matches identical to the reference's (per ordered view pair, ascending pairs, n-major / m-minor); as many seeds per
    view pair; no seed twice within a pair; two different matches per seed, both from the pair's list."""
    from cosypose_amd.multiview_matching import make_ransac_infos, SEED_KEYS
    scene = rc.scene_of(g, prefix)
    seeds, tm = make_ransac_infos(scene['cand_view_id'], labels_of(scene), n_iter, 0)
    for k in ('pair_view1', 'pair_view2', 'pair_off', 'pair_cand1', 'pair_cand2'):
        assert np.array_equal(getattr(tm, k), g[f'{prefix}tm_{k}']), k
    n_pairs = len(tm.pair_view1)
    assert np.array_equal(np.bincount(tm.hyp_pair, minlength=n_pairs), np.bincount(g[prefix + 'tm_hyp_pair'], minlength=n_pairs))
    sizes = tm.pair_sizes
    assert np.array_equal(np.bincount(tm.hyp_pair, minlength=n_pairs), np.minimum(n_iter, sizes * (sizes - 1)))
    assert list(seeds) == list(SEED_KEYS) and all(v.dtype == np.int32 for v in seeds.values())
    assert np.all(np.diff(tm.hyp_pair) >= 0)
    assert np.array_equal(seeds['view1'], tm.pair_view1[tm.hyp_pair]) and np.array_equal(seeds['view2'], tm.pair_view2[tm.hyp_pair])
    rows = np.stack([tm.hyp_pair] + [seeds[k] for k in SEED_KEYS[2:]], 1)
    assert len(np.unique(rows, axis=0)) == len(rows), 'a seed is drawn twice'
    assert np.all((rows[:, 1] != rows[:, 3]) | (rows[:, 2] != rows[:, 4])), 'match 1 == match 2'
    listed = set(zip(np.repeat(np.arange(n_pairs), sizes).tolist(), tm.pair_cand1.tolist(), tm.pair_cand2.tolist()))
    assert all((p, a, b) in listed and (p, c, d) in listed for p, a, b, c, d in rows.tolist())
    view = scene['cand_view_id']
    assert np.array_equal(view[seeds['match1_cand1']], seeds['view1']) and np.array_equal(view[seeds['match2_cand2']], seeds['view2'])


def test_make_ransac_infos_exhaustive_when_small(g):
    """n_tm (n_tm - 1) <= 2000 for every view pair of scene a_: the SET of seeds is the reference's (its order is libstdc++'s)."""
    from cosypose_amd.multiview_matching import make_ransac_infos, SEED_KEYS
    scene = rc.scene_of(g, 'a_')
    seeds, _ = make_ransac_infos(scene['cand_view_id'], labels_of(scene), 2000, 0)
    own = set(zip(*(seeds[k].tolist() for k in SEED_KEYS)))
    ref = set(zip(*(g['a_seed_' + k].tolist() for k in SEED_KEYS)))
    assert len(own) == len(seeds['view1']) == 1012 and own == ref


def test_make_ransac_infos_seed_changes_the_draw_not_the_counts(g):
    from cosypose_amd.multiview_matching import make_ransac_infos
    scene = rc.scene_of(g, 'b_')
    s0, _ = make_ransac_infos(scene['cand_view_id'], labels_of(scene), 50, 0)
    s0b, _ = make_ransac_infos(scene['cand_view_id'], labels_of(scene), 50, 0)
    s1, _ = make_ransac_infos(scene['cand_view_id'], labels_of(scene), 50, 7)
    assert all(np.array_equal(s0[k], s0b[k]) for k in s0)
    assert len(s1['view1']) == len(s0['view1']) and not np.array_equal(s0['match1_cand1'], s1['match1_cand1'])


def test_tentative_matches_expand_and_compact(g):
    """The three reference keys expand to (hypothesis, every match of its pair); compacting the expansion gives the lists back."""
    from cosypose_amd.multiview_matching import _compact_tmatches
    tm = rc.tmatches_of(g, 'b_')
    seeds = rc.seeds_of(g, 'b_')
    assert set(tm) == {'hypothesis_id', 'cand1', 'cand2'} and len(tm['cand1']) == len(g['b_dists'])
    sizes = tm.pair_sizes[tm.hyp_pair]
    assert np.array_equal(np.bincount(tm['hypothesis_id']), sizes)
    h = 1234
    sl = slice(tm.pair_off[tm.hyp_pair[h]], tm.pair_off[tm.hyp_pair[h] + 1])
    assert np.array_equal(tm['cand1'][tm['hypothesis_id'] == h], tm.pair_cand1[sl]) and np.array_equal(tm['cand2'][tm['hypothesis_id'] == h], tm.pair_cand2[sl])
    back = _compact_tmatches(dict(tm), seeds['view1'], seeds['view2'])
    for k in ('pair_view1', 'pair_view2', 'pair_off', 'pair_cand1', 'pair_cand2', 'hyp_pair'):
        assert np.array_equal(getattr(back, k), getattr(tm, k)), k
    bad = dict(tm)
    bad = {k: v[:-1] for k, v in bad.items()}
    with pytest.raises(ValueError, match='different numbers'):
        _compact_tmatches(bad, seeds['view1'], seeds['view2'])


@pytest.mark.parametrize('prefix', ['a_', 'b_'])
def test_scene_level_matching_and_pairs_vs_reference(g, prefix):
    """The reference's inlier matches in -> the reference's filtered candidates (same rows, same partition), scene_infos and view
    pairs out, on CPU tensors."""
    from cosypose_amd.multiview_matching import scene_level_matching, get_best_viewpair_pose_est, make_obj_infos
    cand, _, _ = rc.collections(g, prefix)
    cand.infos['cand_id'] = np.arange(len(cand))
    inliers = dict(inlier_matches_cand1=g[prefix + 'inlier_cand1'], inlier_matches_cand2=g[prefix + 'inlier_cand2'],
                   best_hypotheses=g[prefix + 'best_hypotheses'])
    matched = scene_level_matching(cand, inliers)
    assert list(matched.infos.columns) == ['view_id', 'label', 'score', 'cand_id', 'obj_id']
    obj = matched.infos['obj_id'].values
    assert sorted(set(obj.tolist())) == list(range(obj.max() + 1)) and obj[0] == 0 and np.all(np.diff(np.maximum.accumulate(obj)) <= 1)
    assert torch.equal(matched.poses, cand.poses[matched.infos['cand_id'].values])
    if prefix == 'a_':
        assert np.array_equal(matched.infos['cand_id'].values, g['a_e2e_cand_id'])
        assert rc.partition(obj) == rc.partition(g['a_e2e_obj_id'])
        infos = make_obj_infos(matched)
        key = lambda n, s, l: sorted(zip(np.asarray(n).tolist(), np.round(s, 9).tolist(), np.asarray(l).tolist()))
        assert key(infos['n_cand'], infos['score'], [int(l[4:]) - 1 for l in infos['label']]) == key(g['a_e2e_info_n_cand'], g['a_e2e_info_score'], g['a_e2e_info_label'])
    else:
        truth = rc.scene_of(g, 'b_')['cand_obj_id'][matched.infos['cand_id'].values]
        assert all(len(set(truth[list(p)].tolist())) == 1 for p in rc.partition(obj))      # 50 iterations: objects may be split, never merged
    seeds = rc.seeds_of(g, prefix)
    TC1C2 = torch.from_numpy(g[prefix + 'TC1C2'])
    pairs = get_best_viewpair_pose_est(TC1C2, seeds, inliers)
    assert list(pairs.infos.columns) == ['view1', 'view2']
    assert np.array_equal(pairs.infos['view1'].values, seeds['view1'][inliers['best_hypotheses']])
    assert np.array_equal(pairs.infos['view2'].values, seeds['view2'][inliers['best_hypotheses']])
    assert torch.equal(pairs.TC1C2, TC1C2[inliers['best_hypotheses'].astype(np.int64)])
    if prefix == 'a_':
        assert np.array_equal(pairs.infos['view1'].values, g['a_e2e_view1']) and np.array_equal(pairs.infos['view2'].values, g['a_e2e_view2'])


def test_scene_level_matching_needs_both_directions():
    """cand 0 -> 1 and 1 -> 0 make an object; 2 -> 3 alone does not (the components are STRONG); singletons are dropped."""
    from cosypose_amd.multiview_matching import scene_level_matching
    from cosypose_amd.tensor_collection import PandasTensorCollection
    cand = PandasTensorCollection(pd.DataFrame(dict(view_id=[0, 1, 0, 1, 2], label=['x'] * 5, score=[0.5] * 5, cand_id=np.arange(5))),
                                  poses=torch.eye(4).repeat(5, 1, 1) * torch.arange(1, 6).view(5, 1, 1))
    out = scene_level_matching(cand, dict(inlier_matches_cand1=np.array([0, 1, 2]), inlier_matches_cand2=np.array([1, 0, 3])))
    assert out.infos['cand_id'].tolist() == [0, 1] and out.infos['obj_id'].tolist() == [0, 0]
    assert torch.equal(out.poses, cand.poses[:2])


def empty_checks(out, n_cols):
    assert len(out['filtered_candidates']) == 0 and out['filtered_candidates'].poses.shape == (0, 4, 4)
    assert list(out['filtered_candidates'].infos.columns) == n_cols + ['cand_id', 'obj_id']
    assert len(out['pairs_TC1C2']) == 0 and out['pairs_TC1C2'].TC1C2.shape == (0, 4, 4) and list(out['pairs_TC1C2'].infos.columns) == ['view1', 'view2']
    assert len(out['scene_infos']) == 0 and set(out['scene_infos'].columns) == {'obj_id', 'score', 'label', 'n_cand'}
    assert all(out[k] >= 0 for k in ('time_models', 'time_score', 'time_misc'))


def test_empty_cases_without_a_device(g):
    """A single view, and views that share no label: no tentative match, so no launch -- empty collections with the right columns
    (CPU tensors suffice: nothing reaches the library)."""
    from cosypose_amd.multiview_matching import multiview_candidate_matching, make_ransac_infos
    cand, _, mesh_db = rc.collections(g, 'a_')
    one_view = cand[np.where(cand.infos['view_id'] == cand.infos['view_id'][0])[0]]
    empty_checks(multiview_candidate_matching(one_view, mesh_db, n_ransac_iter=50), ['view_id', 'label', 'score'])
    views = cand.infos['view_id'].values
    labels = cand.infos['label'].values
    keep = np.where(((views == views[0]) & (labels == 'obj_000001')) | ((views == views[-1]) & (labels != 'obj_000001')))[0]
    apart = cand[keep]
    assert len(set(apart.infos['view_id'])) == 2
    empty_checks(multiview_candidate_matching(apart, mesh_db, n_ransac_iter=50), ['view_id', 'label', 'score'])
    seeds, tm = make_ransac_infos([], [], 10, 0)
    assert all(len(v) == 0 for v in seeds.values()) and len(tm['cand1']) == 0
    # one tentative match in a pair: no seed (two different matches are needed)
    seeds, tm = make_ransac_infos([0, 1], ['x', 'x'], 10, 0)
    assert len(seeds['view1']) == 0 and tm.pair_sizes.tolist() == [1, 1]


def test_predictor_with_nothing_matched(g):
    """One view: no object can be matched; predict_scene_state returns the reference's keys with empty collections (no launch)."""
    from cosypose_amd.multiview_predictor import MultiviewScenePredictor
    cand, cams, mesh_db = rc.collections(g, 'a_')
    cand = cand[np.where(cand.infos['view_id'] == cand.infos['view_id'][0])[0]]
    cand.infos['scene_id'], cand.infos['group_id'] = 1, 0
    cams.infos['scene_id'], cams.infos['batch_im_id'] = 1, np.arange(len(cams))
    pred = MultiviewScenePredictor(mesh_db.aabb(), mesh_db).predict_scene_state(cand, cams)
    assert {'cand_inputs', 'cand_matched', 'scene/objects', 'scene/cameras', 'ba_input', 'ba_output', 'ba_output+all_cand'} <= set(pred)
    assert len(pred['cand_inputs']) == len(cand) == len(pred['ba_output+all_cand'])
    assert all(len(pred[k]) == 0 for k in ('cand_matched', 'scene/objects', 'scene/cameras', 'ba_input', 'ba_output'))


def test_aabb_corner_order():
    """BatchedMeshes.aabb(): the 8 corners in the reference's order (mesh_ops.py:15-28), symmetries and labels kept."""
    from cosypose_amd.mesh_db import BatchedMeshes
    pts = torch.tensor([[[0., 0, 0], [1, 2, 3], [-1, 5, 2], [0.5, -2, 1]]])
    db = BatchedMeshes({'x': dict(label='x', n_sym=1)}, ['x'], pts, torch.eye(4)[None, None]).aabb()
    want = [[-1, 5, 3], [1, 5, 3], [1, -2, 3], [-1, -2, 3], [-1, 5, 0], [1, 5, 0], [1, -2, 0], [-1, -2, 0]]
    assert db.points.tolist() == [[[float(v) for v in row] for row in want]] and db.labels.tolist() == ['x'] and db.symmetries.shape == (1, 1, 4, 4)


def test_ids_are_checked_on_the_host(g):
    from cosypose_amd.multiview_matching import _seed_table, multiview_candidate_matching
    seeds = rc.seeds_of(g, 'a_')
    bad = dict(seeds, match2_cand2=np.where(np.arange(len(seeds['view1'])) == 5, 21, seeds['match2_cand2']))
    with pytest.raises(ValueError, match=r'outside \[0, 21\)'):
        _seed_table(bad, 21)
    cand, _, mesh_db = rc.collections(g, 'a_')
    with pytest.raises(ValueError, match='no tentative matches'):
        multiview_candidate_matching(cand, mesh_db, seeds=dict(seeds, view1=seeds['view1'] + 1000))


def test_new_symbols_declared_bound_and_exported():
    from cosypose_amd import _lib
    from cosypose_amd.build import build, SOURCES
    build()
    for name in ('cosy_ransac_max_tmatches', 'cosy_ransac_hypotheses', 'cosy_ransac_score', 'cosy_ransac_best'):
        assert name in _lib.EXPORTS           # test_c_abi.py: EXPORTS, the header and the built library name the same entry points
    assert 'kernels_ransac.hip' in SOURCES
    import cosypose_amd
    from cosypose_amd import multiview_matching, multiview_predictor
    assert cosypose_amd.multiview_candidate_matching is multiview_matching.multiview_candidate_matching
    assert cosypose_amd.MultiviewScenePredictor is multiview_predictor.MultiviewScenePredictor
    assert multiview_matching.score_tmatches_batch is multiview_matching.score_tmaches_batch       # both spellings
    assert _lib.lib().cosy_ransac_max_tmatches() >= 1024
    # argument checks that need no device
    l = _lib.lib()
    n = [None] * 4
    assert l.cosy_ransac_score(*n, 0, 0, 0, 0, None, None, 0, None, None, 0, 5000, 0.0, None, None, None, None, None, None) == -4
    assert b'5000' in l.cosy_last_error()
    assert l.cosy_ransac_hypotheses(*n, None, 1, 1, 8, 65, None, 1, None, None, None, None, None) in (-1, -4)
    assert l.cosy_ransac_hypotheses(*n, None, 0, 0, 0, 0, None, 0, None, None, None, None, None) == 0
