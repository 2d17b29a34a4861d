"""Shared by test_multiview_matching.py / test_multiview_matching_host.py: the fixture of tests/golden/generate_golden_ransac.py as
this package's collections."""
import pathlib

import numpy as np
import torch

HERE = pathlib.Path(__file__).resolve().parent
SEED_KEYS = ('view1', 'view2', 'match1_cand1', 'match1_cand2', 'match2_cand1', 'match2_cand2')
INPUTS_OF = dict(a_='a_', b_='b_', c_='b_', d_='d_', k_='a_', e_='e_')      # c_ / k_ reuse the scene of b_ / a_


def load():
    return dict(np.load(HERE / 'golden' / 'reference_golden_ransac.npz', allow_pickle=False))


def scene_of(g, prefix):
    key = INPUTS_OF[prefix] + 'in_'
    return {k[len(key):]: v for k, v in g.items() if k.startswith(key)}


def collections(g, prefix, device='cpu', dtype=torch.float32):
    """(candidates without obj_id, cameras with TWC, mesh_db of the 8 box corners) of a fixture scene"""
    from cosypose_amd import synthetic as syn
    from cosypose_amd.mesh_db import BatchedMeshes
    scene = scene_of(g, prefix)
    scene.update(pair_view1=np.zeros(0, np.int64), pair_view2=np.zeros(0, np.int64), pair_TC1C2=np.zeros((0, 4, 4)))
    cand, cams, _, mesh_db = syn.ba_scene_collections(scene, BatchedMeshes, dtype=dtype, device=device)
    cand.infos = cand.infos.drop(columns=['obj_id'])
    cams.register_tensor('TWC', torch.as_tensor(scene['cam_TWC']).to(dtype).to(device))
    return cand, cams, mesh_db


def seeds_of(g, prefix):
    return {k: g[f'{prefix}seed_{k}'] for k in SEED_KEYS}


def tmatches_of(g, prefix):
    from cosypose_amd.multiview_matching import TentativeMatches
    return TentativeMatches(*(g[f'{prefix}tm_{k}'] for k in ('pair_view1', 'pair_view2', 'pair_off', 'pair_cand1', 'pair_cand2', 'hyp_pair')))


def partition(ids):
    groups = {}
    for n, i in enumerate(np.asarray(ids).tolist()):
        groups.setdefault(i, []).append(n)
    return sorted(tuple(v) for v in groups.values())
