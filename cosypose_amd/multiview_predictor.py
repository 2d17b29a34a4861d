"""Scene reconstruction from per-view candidates (CosyPose stages 2 + 3), same surface as the reference's
cosypose/integrated/multiview_predictor.py:14-127: candidate matching (multiview_matching.py), one bundle adjustment per group of
connected views (bundle_adjustment.py), and the refined objects reprojected into every view.

The constructor takes the two BatchedMeshes instead of a MeshDataBase (loading meshes from .ply is out of scope, mesh_db.py):
`mesh_db_ransac` holds the 8 bounding-box corners per object (BatchedMeshes.aabb()), `mesh_db_ba` the points of the bundle adjustment."""
import numpy as np
import pandas as pd

from . import tensor_collection as tc
from .bundle_adjustment import MultiviewRefinement, make_view_groups, invert_T, solve_problems
from .multiview_matching import multiview_candidate_matching


class MultiviewScenePredictor:
    def __init__(self, mesh_db_ransac, mesh_db_ba=None):
        self.mesh_db_ransac = mesh_db_ransac
        self.mesh_db_ba = mesh_db_ba if mesh_db_ba is not None else mesh_db_ransac

    def reproject_scene(self, objects, cameras):
        """Every object in every camera: TCO = inv(TWC) TWO, rows object-major / view-minor with the reference's columns (:20-41), as
        ONE batched product instead of one collection per (object, view)."""
        n_obj, n_cam = len(objects), len(cameras)
        obj = lambda k: np.repeat(objects.infos[k].values, n_cam)
        cam = lambda k: np.tile(cameras.infos[k].values, n_obj)
        infos = pd.DataFrame(dict(scene_id=cam('scene_id'), view_id=cam('view_id'), score=obj('score') + 1.0, view_group=obj('view_group'),
                                  label=obj('label'), batch_im_id=cam('batch_im_id'), obj_id=obj('obj_id'), from_ba=np.ones(n_obj * n_cam, bool)))
        poses = (invert_T(cameras.TWC)[None, :] @ objects.TWO[:, None]).reshape(n_obj * n_cam, 4, 4)
        return tc.PandasTensorCollection(infos=infos, poses=poses)

    def _match_scene(self, candidates, cameras, score_th, use_known_camera_poses, ransac_n_iter, ransac_dist_threshold):
        """Stage 2 on one scene -> (predictions so far, the matched candidates with their view_group, pairs_TC1C2, scene_id, group_id)"""
        predictions = dict()
        assert len(np.unique(candidates.infos['scene_id'])) == 1
        scene_id = np.unique(candidates.infos['scene_id']).item()
        group_id = np.unique(candidates.infos['group_id']).item()
        keep = np.where(candidates.infos['score'] >= score_th)[0]
        candidates = candidates[keep]
        predictions['cand_inputs'] = candidates

        matching_outputs = multiview_candidate_matching(
            candidates=candidates, mesh_db=self.mesh_db_ransac, n_ransac_iter=ransac_n_iter, dist_threshold=ransac_dist_threshold,
            cameras=cameras if use_known_camera_poses else None)
        pairs_TC1C2 = matching_outputs['pairs_TC1C2']
        candidates = matching_outputs['filtered_candidates']
        predictions['cand_matched'] = candidates
        predictions['matching'] = {k: v for k, v in matching_outputs.items() if k.startswith('time_')}

        group_infos = make_view_groups(pairs_TC1C2)
        candidates = candidates.merge_df(group_infos, on='view_id')
        return predictions, candidates, pairs_TC1C2, scene_id, group_id

    def _view_group_problems(self, candidates, cameras, pairs_TC1C2):
        """[(view_group, MultiviewRefinement), ...] of a scene's matched candidates"""
        return [(view_group, MultiviewRefinement(candidates=candidates[np.asarray(candidate_ids)], cameras=cameras, pairs_TC1C2=pairs_TC1C2,
                                                 mesh_db=self.mesh_db_ba))
                for view_group, candidate_ids in candidates.infos.groupby('view_group').groups.items()]

    def _scene_predictions(self, predictions, cand_inputs, group_outputs, scene_id, group_id):
        """group_outputs: [(view_group, the solve's outputs), ...] of one scene -> its predictions, completed"""
        pred_objects, pred_cameras, pred_reproj, pred_reproj_init, histories = [], [], [], [], []
        for view_group, ba_outputs in group_outputs:
            scenes = []
            for key_o, key_c in (('objects', 'cameras'), ('objects_init', 'cameras_init')):
                objects_, cameras_ = ba_outputs[key_o], ba_outputs[key_c]
                for x in (objects_, cameras_):
                    # the frames are shared between the solve's outputs: every state gets its own before it is labelled
                    x.infos = x.infos.assign(view_group=view_group, group_id=group_id, scene_id=scene_id)
                scenes.append((objects_, cameras_))
            pred_reproj.append(self.reproject_scene(*scenes[0]))
            pred_reproj_init.append(self.reproject_scene(*scenes[1]))
            pred_objects.append(scenes[0][0])
            pred_cameras.append(scenes[0][1])
            histories.append(ba_outputs['history'])

        predictions['scene/objects'] = tc.concatenate(pred_objects)
        predictions['scene/cameras'] = tc.concatenate(pred_cameras)
        predictions['ba_output'] = tc.concatenate(pred_reproj)
        predictions['ba_input'] = tc.concatenate(pred_reproj_init)
        predictions['ba_history'] = histories
        cand_inputs = tc.PandasTensorCollection(infos=cand_inputs.infos, poses=cand_inputs.poses)
        predictions['ba_output+all_cand'] = tc.concatenate([predictions['ba_output'], cand_inputs])
        return predictions

    def predict_scene_state(self, candidates, cameras, score_th=0.3, use_known_camera_poses=False, ransac_n_iter=2000,
                            ransac_dist_threshold=0.02, ba_n_iter=100):
        """candidates: infos scene_id, group_id, view_id, label, score + poses (n,4,4) on the device, all of one scene; cameras: infos
        scene_id, view_id, batch_im_id + K (and TWC with use_known_camera_poses).  -> dict with the reference's keys: cand_inputs,
        cand_matched, scene/objects, scene/cameras, ba_input, ba_output, ba_output+all_cand."""
        predictions, matched, pairs_TC1C2, scene_id, group_id = self._match_scene(candidates, cameras, score_th, use_known_camera_poses,
                                                                                 ransac_n_iter, ransac_dist_threshold)
        group_outputs = [(view_group, problem.solve(n_iterations=ba_n_iter, optimize_cameras=not use_known_camera_poses))
                         for view_group, problem in self._view_group_problems(matched, cameras, pairs_TC1C2)]
        return self._scene_predictions(predictions, candidates, group_outputs, scene_id, group_id)

    def predict_scene_states(self, scenes, score_th=0.3, use_known_camera_poses=False, ransac_n_iter=2000, ransac_dist_threshold=0.02,
                             ba_n_iter=100, ba_history=False):
        """predict_scene_state of every (candidates, cameras) of `scenes` -> list of its dicts.  The matching runs per scene, unchanged;
        the view groups of ALL scenes then go through ONE bundle_adjustment.solve_problems call (they share mesh_db_ba), so that the
        bundle adjustment costs one set of launches per iteration instead of one per view group.  ba_history: keep the 9-D states of
        every history entry (predict_scene_state's histories also hold the converted `objects` / `cameras`; these do not)."""
        matched = [self._match_scene(candidates, cameras, score_th, use_known_camera_poses, ransac_n_iter, ransac_dist_threshold)
                   for candidates, cameras in scenes]
        groups = [self._view_group_problems(m[1], cameras, m[2]) for m, (_, cameras) in zip(matched, scenes)]
        outputs = solve_problems([problem for scene_groups in groups for _, problem in scene_groups], n_iterations=ba_n_iter,
                                 optimize_cameras=not use_known_camera_poses, history=ba_history)
        results, first = [], 0
        for (predictions, _, _, scene_id, group_id), scene_groups, (candidates, _) in zip(matched, groups, scenes):
            group_outputs = [(view_group, out) for (view_group, _), out in zip(scene_groups, outputs[first:first + len(scene_groups)])]
            first += len(scene_groups)
            results.append(self._scene_predictions(predictions, candidates, group_outputs, scene_id, group_id))
        return results
