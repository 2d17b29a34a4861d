"""Shared by test_bundle_adjustment_batch.py / test_bundle_adjustment_batch_host.py: sub-problems of ONE synthetic.make_ba_scene scene
(its mesh table depends on the seed, so problems of different seeds cannot share a mesh_db) as MultiviewRefinement instances on one
mesh_db."""
import numpy as np
import torch

NAN_MESH = 4        # row of the extra mesh with n_sym = 0 that `with_nan_mesh` appends: a candidate that names it aligns to NaN


def sub_scene(scene, views, objects):
    """The candidates, cameras and pairs of `scene` that lie in `views` (indices into its cameras) and `objects` (indices into its
    sorted object ids); the mesh tables are kept."""
    view_ids = scene['cam_view_id'][np.asarray(views)]
    obj_ids = np.unique(scene['cand_obj_id'])[np.asarray(objects)]
    cand = np.isin(scene['cand_view_id'], view_ids) & np.isin(scene['cand_obj_id'], obj_ids)
    cam = np.isin(scene['cam_view_id'], view_ids)
    pair = np.isin(scene['pair_view1'], view_ids) & np.isin(scene['pair_view2'], view_ids)
    out = dict(scene)
    out.update({k: v[cand] for k, v in scene.items() if k.startswith('cand_')})
    out.update({k: v[cam] for k, v in scene.items() if k.startswith('cam_')})
    out.update({k: v[pair] for k, v in scene.items() if k.startswith('pair_')})
    return out


def with_nan_mesh(scene):
    """`scene` with a fifth mesh (the points and symmetries of mesh 0) whose n_sym is 0; no candidate names it yet"""
    out = dict(scene)
    out.update(pts=np.concatenate([scene['pts'], scene['pts'][:1]]), sym=np.concatenate([scene['sym'], scene['sym'][:1]]),
               n_sym=np.concatenate([scene['n_sym'], [0]]).astype(np.int32))
    assert len(out['n_sym']) == NAN_MESH + 1
    return out


def nan_scene(scene):
    """every candidate of `scene` (made by with_nan_mesh) names the mesh without a symmetry: the loss is NaN from the first linearisation"""
    out = dict(scene)
    out['cand_label_id'] = np.full_like(scene['cand_label_id'], NAN_MESH)
    return out


def mesh_db_of(scene, device=None, dtype=torch.float64):
    from cosypose_amd import synthetic as syn
    from cosypose_amd.mesh_db import BatchedMeshes
    return syn.ba_scene_collections(scene, BatchedMeshes, dtype=dtype, device=device)[3]


def problem_on(scene, mesh_db, device=None, dtype=torch.float64):
    """MultiviewRefinement of a (sub-)scene on the SHARED mesh_db"""
    from cosypose_amd import synthetic as syn
    from cosypose_amd.bundle_adjustment import MultiviewRefinement
    return MultiviewRefinement(*syn.ba_scene_collections(scene, lambda *a: mesh_db, dtype=dtype, device=device))
