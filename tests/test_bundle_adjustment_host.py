"""Host side of the bundle adjustment (cosypose_amd/bundle_adjustment.py) against the reference's outputs in
tests/golden/reference_golden_ba.npz (tests/golden/generate_golden_ba.py).  No GPU and no libcosyhip.so: the constructor and the
initialisation walk are pandas / numpy code.  Also pins tests/ba_ref.py, the float64 reference of the GPU tests, to the reference's
stored autograd runs."""
import pathlib

import numpy as np
import pandas as pd
import pytest
import torch

import ba_ref
from cosypose_amd import bundle_adjustment as ba
from cosypose_amd import synthetic as syn
from cosypose_amd.mesh_db import BatchedMeshes
from cosypose_amd.tensor_collection import PandasTensorCollection

GOLDEN = pathlib.Path(__file__).resolve().parent / 'golden' / 'reference_golden_ba.npz'
SCENES = ('s1_', 's2_', 's3_', 's4_', 's5_', 'f2_', 'f4_')


@pytest.fixture(scope='module')
def golden():
    return dict(np.load(GOLDEN, allow_pickle=False))


def scene_inputs(g, prefix):
    key = prefix + 'in_'
    return {k[len(key):]: v for k, v in g.items() if k.startswith(key)}


def test_make_view_groups_partition(golden):
    g = golden
    pairs = PandasTensorCollection(pd.DataFrame(dict(view1=g['vg_view1'], view2=g['vg_view2'])), TC1C2=torch.eye(4).repeat(len(g['vg_view1']), 1, 1))
    got = ba.make_view_groups(pairs)
    assert list(got.columns) == ['view_id', 'view_group']
    assert np.array_equal(got['view_id'].values, g['vg_view_id'])

    def partition(ids, groups):
        return {frozenset(ids[groups == k].tolist()) for k in np.unique(groups)}
    want = partition(g['vg_view_id'], g['vg_view_group'])
    assert partition(got['view_id'].values, got['view_group'].values) == want
    assert len(want) == 4 and frozenset([30]) in want and frozenset([31]) in want      # the one-way edge 30 -> 31 joins nothing


def test_strong_components_cycle_and_chain():
    comp = ba._strong_components(6, [(0, 1), (1, 2), (2, 0), (2, 3), (3, 4), (4, 3), (5, 5)])
    assert comp[0] == comp[1] == comp[2] and comp[3] == comp[4] and len({comp[0], comp[3], comp[5]}) == 3


@pytest.mark.parametrize('prefix', SCENES)
def test_make_obj_infos_vs_reference(golden, prefix):
    g = golden
    cand, _, _, _ = syn.ba_scene_collections(scene_inputs(g, prefix), BatchedMeshes)
    got = ba.make_obj_infos(cand)
    assert list(got.columns) == g[prefix + 'objinfo_columns'].tolist()
    assert np.array_equal(got['obj_id'].values, g[prefix + 'objinfo_obj_id'])
    assert np.array_equal(got['n_cand'].values, g[prefix + 'objinfo_n_cand'])
    assert np.array_equal([int(l[4:]) - 1 for l in got['label']], g[prefix + 'objinfo_label'])
    assert np.abs(got['score'].values - g[prefix + 'objinfo_score']).max() < 1e-14


@pytest.mark.parametrize('prefix', SCENES)
def test_constructor_maps_and_initialisation_on_cpu_tensors(golden, prefix):
    g = golden
    cand, cams, pairs, mesh_db = syn.ba_scene_collections(scene_inputs(g, prefix), BatchedMeshes)
    p = ba.MultiviewRefinement(cand, cams, pairs, mesh_db)
    assert (p.n_views, p.n_objects, p.n_candidates) == (len(g[prefix + 'in_cam_view_id']), len(g[prefix + 'objinfo_obj_id']), len(cand))
    assert p.cand_obj_ids == g[prefix + 'obj_ids'].tolist() and p.cand_view_ids == g[prefix + 'view_ids'].tolist()
    assert np.array_equal(p.visibility_matrix.numpy(), g[prefix + 'visibility']) and p.visibility_matrix.dtype == torch.int32
    assert sorted(p.v2v1_pair_row) == [tuple(k) for k in g[prefix + 'v2v1_keys'].tolist()]
    TC2C1 = p._host_state()['TC2C1']
    for key, want in zip(g[prefix + 'v2v1_keys'].tolist(), g[prefix + 'v2v1_TC2C1']):
        assert np.abs(TC2C1[p.v2v1_pair_row[tuple(key)]] - want).max() < 1e-15
    assert p.K.shape == (p.n_views, 3, 3) and p.K.dtype == torch.float64
    TWO, TWC = p.sample_initial_TWO_TWC(0)       # the walk over the view graph is host code: same permutations as the reference
    assert np.abs(TWO.numpy() - g[prefix + 'TWO_init']).max() <= 1e-12
    assert np.abs(TWC.numpy() - g[prefix + 'TWC_init']).max() <= 1e-12


def test_constructor_rejects_empty_and_cameraless_input(golden):
    scene = scene_inputs(golden, 's1_')
    cand, cams, pairs, mesh_db = syn.ba_scene_collections(scene, BatchedMeshes)
    with pytest.raises(ValueError, match='no candidates'):
        ba.MultiviewRefinement(cand[np.arange(0)], cams, pairs, mesh_db)
    with pytest.raises(ValueError, match='view_id'):
        ba.MultiviewRefinement(cand, cams[np.arange(1, len(cams))], pairs, mesh_db)


def test_sampler_error_for_a_view_without_pair_path(golden):
    scene = scene_inputs(golden, 's3_')
    lone = scene['cam_view_id'][2]
    keep = (scene['pair_view1'] != lone) & (scene['pair_view2'] != lone)
    for k in ('pair_view1', 'pair_view2', 'pair_TC1C2'):
        scene[k] = scene[k][keep]
    p = ba.MultiviewRefinement(*syn.ba_scene_collections(scene, BatchedMeshes))
    with pytest.raises(ba.SamplerError):
        p.sample_initial_TWO_TWC(0)


GOLDEN_JAC = GOLDEN.with_name('reference_golden_ba_jac.npz')
LIN_CEILING = 1e-9       # as in test_bundle_adjustment.py: anything above is not float64 in another order
# 10 x the worst max |got - want| / max |want| of ba_ref against the stored runs over the six states: errors 8.5e-14, loss 8.6e-15,
# J_TWO / J_TCW 4.7e-16, align distances 4.9e-15
REF_TOL = dict(errors=8.5e-13, loss=8.6e-14, J_TWO=4.7e-15, J_TCW=4.7e-15, align_dists=4.9e-14)


@pytest.mark.parametrize('prefix,tag', [(s, tag) for s in ('s1_', 's2_', 's4_') for tag in ('init', 'final')])
def test_ba_ref_vs_stored_autograd_runs(golden, prefix, tag):
    """tests/ba_ref.py, the float64 reference that tests/test_ba_kernels.py holds the kernels to, against the reference project's own
    stored float64 autograd runs at the initial and final states of scenes 1, 2, 4: errors, loss, the compact Jacobian, and at the
    initial states (where they are stored) the align distances and chosen symmetries.  A wrong reference cannot hide a wrong kernel."""
    g = dict(golden)
    g.update(np.load(GOLDEN_JAC, allow_pickle=False))
    r = ba_ref.reference(g[f'{prefix}TWO_9d_{tag}'], g[f'{prefix}TCW_9d_{tag}'], g[prefix + 'in_cand_poses'], g[prefix + 'in_cam_K'],
                         g[prefix + 'obj_ids'], g[prefix + 'view_ids'], g[prefix + 'in_cand_label_id'], g[prefix + 'objinfo_label'],
                         g[prefix + 'in_pts'], g[prefix + 'in_sym'], g[prefix + 'in_n_sym'], 25)

    def rel(got, want):
        return float(np.abs(np.asarray(got) - want).max() / np.abs(want).max())
    figs = {k: rel(r[k], g[f'{prefix}{tag}_{k}']) for k in ('errors', 'loss', 'J_TWO', 'J_TCW')}
    if tag == 'init':
        figs['align_dists'] = rel(r['dists'][np.arange(len(r['best'])), r['best']], g[prefix + 'align_dists'])
        assert np.array_equal(r['best'], g[prefix + 'align_sym'])
        assert rel(r['aligned'], g[prefix + 'align_TCO']) < LIN_CEILING
        assert r['margin'].min() >= 1e-3                     # the fixture generator's own rule
    print(f'FIGURE ba_ref vs stored run {prefix}{tag}', figs)
    for k, v in figs.items():
        assert v <= min(REF_TOL[k], LIN_CEILING), figs
    # the dense forms are the compact ones scattered: A and b from them
    J, e = r['J'], r['errors']
    assert J.shape == (len(e), 9 * (len(g[prefix + 'objinfo_obj_id']) + len(g[prefix + 'in_cam_view_id'])))
    rows, per_cand = np.arange(len(e))[:, None], len(e) // len(g[prefix + 'obj_ids'])
    cols_o = np.repeat(g[prefix + 'obj_ids'], per_cand)[:, None] * 9 + np.arange(9)
    cols_v = (len(g[prefix + 'objinfo_obj_id']) + np.repeat(g[prefix + 'view_ids'], per_cand))[:, None] * 9 + np.arange(9)
    assert np.array_equal(J[rows, cols_o], r['J_TWO']) and np.array_equal(J[rows, cols_v], r['J_TCW'])
    assert np.count_nonzero(J) == np.count_nonzero(r['J_TWO']) + np.count_nonzero(r['J_TCW'])
    assert rel(r['A'], J.T @ J) < 1e-14 and np.abs(r['b'] - J.T @ e).max() <= 1e-14 * np.abs(r['b_scale']).max()
