#!/usr/bin/env python3
"""Generate tests/golden/reference_golden_ba.npz and reference_golden_ba_jac.npz: the REFERENCE's own bundle adjustment
(cosypose/multiview/bundle_adjustment.py, run in place, FLOAT64 on the CPU, one thread) on seeded synthetic scenes
(cosypose_amd.synthetic.make_ba_scene).  Run in the build container only:   python tests/golden/generate_golden_ba.py

Shims, next to generate_golden.install_stubs (which supplies the import stubs and the path of the reference):
  * np.int = int                (multiview/ransac.py:122 uses the alias numpy dropped);
  * torch.Tensor.cuda = identity (bundle_adjustment.py:221 moves the pseudo-inverse back to the GPU);
  * torch.set_num_threads(1)     (bit-stable sums).
The fixtures hold arrays and id / label columns only.  The Jacobians go to a file of their own (compact form: the 9 derivatives
with respect to the residual's own object and own view; the generator asserts that every other entry of the reference's dense
gradients is exactly 0), which keeps each file under the size limit for committed files.

The generator ASSERTS what makes the fixtures worth testing against (see check_run): both branches of the loop are taken, no
accept / reject / stop decision and no choice of symmetry is within rounding of its threshold, and the reference reproduces its own
loss history and relative poses within the tests' ceiling when only its operation order changes.  If a seed violates one of them,
change the seed, not the bound.
"""
import io
import sys
import pathlib
import zipfile

HERE = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import numpy as np
import torch

import generate_golden as gg
from cosypose_amd import synthetic as syn

SCENES = {1: (161, 3, 3, 40), 2: (162, 6, 4, 60), 3: (103, 10, 5, 80), 4: (164, 12, 8, 8), 5: (45, 20, 8, 8)}   # seed, objects, views, points
JACOBIAN_SCENES = (1, 2, 4)
FIXED_CAMERA_SCENES = (2, 4)            # with EXACT view pairs (with the noisy ones the reference accepts no step: nothing to test)
EPS = 1e-5                              # optimize_lm's default
SELF_CEILING = 1e-6                     # = SOLVE_CEILING of tests/test_bundle_adjustment.py


def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def reference():
    gg.install_stubs()
    sys.path.insert(0, str(gg.REPO / 'oracle' / '_ref'))
    np.int = int
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.set_num_threads(1)
    import cosypose_cext  # noqa: F401
    from cosypose.lib3d.rigid_mesh_database import BatchedMeshes
    from cosypose.lib3d import symmetric_distances as sdist
    from cosypose.lib3d.transform_ops import invert_T
    from cosypose.multiview import bundle_adjustment as ba
    from cosypose.multiview.ransac import make_obj_infos
    import cosypose.utils.tensor_collection as tc
    return dict(BatchedMeshes=BatchedMeshes, sdist=sdist, invert_T=invert_T, ba=ba, make_obj_infos=make_obj_infos, tc=tc)


def compact_jacobian(J, ids):
    """dense (n_res, n_blocks, 9) -> (n_res, 9) at the residual's own block; everything else must be exactly 0"""
    J = J.numpy()
    rows = np.arange(J.shape[0])
    own = J[rows, ids].copy()
    rest = J.copy()
    rest[rows, ids] = 0
    assert not rest.any(), 'the reference Jacobian has an entry outside the residual\'s own block'
    return own


def replay_decisions(name, spy_losses, hist_loss, min_accept):
    """optimize_lm's loop walked again over the losses of every linearisation it made (the history alone does not hold the loss of
    a rejected trial step): counts of accepted / rejected steps and the smallest distance of a decision from its threshold"""
    it = iter(spy_losses)
    loss, prev_update, done, accepted, rejected, worst = None, False, False, 0, 0, np.inf
    for n in range(len(hist_loss)):
        if not prev_update:
            loss = next(it)
        assert loss == hist_loss[n]
        if done:
            break
        nxt = next(it)
        rho = loss - nxt
        worst = min(worst, abs(abs(rho) - EPS))
        if abs(rho) < EPS:
            done = True
        elif rho > EPS:
            loss, prev_update, accepted = nxt, True, accepted + 1
        else:
            prev_update, rejected = False, rejected + 1
    assert next(it, None) is None
    print(f'  {name}: {len(hist_loss)} entries, {accepted} accepted, {rejected} rejected, min ||rho| - eps| = {worst:.3g}')
    assert accepted >= min_accept, (name, 'accepted', accepted)
    assert worst >= 1e-7, (name, 'a decision within 1e-7 of eps', worst)
    return accepted, rejected, worst


def run_scene(R, scene, out, prefix, jacobian, optimize_cameras=True, min_accept=3):
    ba = R['ba']
    cand, cams, pairs, mesh_db = syn.ba_scene_collections(scene, R['BatchedMeshes'], collection=R['tc'].PandasTensorCollection)
    mesh_db = mesh_db.double()
    for k, v in scene.items():
        out[prefix + 'in_' + k] = v
    problem = ba.MultiviewRefinement(cand, cams, pairs, mesh_db)
    margins = []
    orig_fj = problem.forward_jacobian

    def spy(TWO_9d, TCW_9d, thr):           # every linearisation's loss, to recover rho of the REJECTED steps too
        res = orig_fj(TWO_9d, TCW_9d, thr)
        margins.append(float(res[1].detach()))
        return res
    problem.forward_jacobian = spy
    res = problem.solve(sample_n_init=1, optimize_cameras=optimize_cameras)
    problem.forward_jacobian = orig_fj
    h = res['history']
    hist_loss = np.array([float(l) for l in h['loss']])
    hist_lambda = np.array(h['lambda'], np.float64)
    accepted, rejected, worst = replay_decisions(prefix, margins, hist_loss, min_accept)
    out[prefix + 'decision_margin'] = np.array(worst)
    out[prefix + 'n_accepted'] = np.array(accepted); out[prefix + 'n_rejected'] = np.array(rejected)
    out[prefix + 'hist_loss'] = hist_loss; out[prefix + 'hist_lambda'] = hist_lambda
    out[prefix + 'hist_iteration'] = np.array(h['iteration'], np.int64)
    out[prefix + 'hist_TCW_9d'] = torch.stack(h['TCW_9d']).numpy()
    out[prefix + 'TWO_init'] = res['objects_init'].TWO.numpy(); out[prefix + 'TWC_init'] = res['cameras_init'].TWC.numpy()
    out[prefix + 'TWO'] = res['objects'].TWO.numpy(); out[prefix + 'TWC'] = res['cameras'].TWC.numpy()
    TCO = R['invert_T'](res['cameras'].TWC)[problem.cand_view_ids] @ res['objects'].TWO[problem.cand_obj_ids]
    out[prefix + 'rel_TCO'] = TCO.numpy()
    # How well does the reference determine its own outputs?  The same run with the unknowns of every step's normal equations
    # permuted (the same pseudo-inverse on P A P^T: nothing but the operation order changes) must take the same decisions and
    # reproduce the loss history and the relative poses within the ceiling the tests apply (SELF_CEILING); a scene that does not
    # (the step along the weakly determined directions is rounding noise amplified by cond(A + lambda I) ~ 1e12) cannot serve.
    def permuted_step(errors, J, lambd):
        A = J.t() @ J + lambd * problem.idJ
        b = J.t() @ errors.view(-1, 1)
        perm = torch.randperm(A.shape[0], generator=torch.Generator().manual_seed(0))
        h = torch.zeros_like(b)
        h[perm] = torch.pinverse(A[perm][:, perm]) @ b[perm]
        return h.flatten()
    problem.compute_lm_step = permuted_step
    res2 = problem.solve(sample_n_init=1, optimize_cameras=optimize_cameras)
    del problem.compute_lm_step
    assert res2['history']['lambda'] == h['lambda'], (prefix, 'the permuted run takes other decisions')
    loss2 = np.array([float(l) for l in res2['history']['loss']])
    TCO2 = R['invert_T'](res2['cameras'].TWC)[problem.cand_view_ids] @ res2['objects'].TWO[problem.cand_obj_ids]
    self_loss = float(np.abs(loss2 - hist_loss).max() / np.abs(hist_loss).max())
    self_TCO = float((TCO2 - TCO).abs().max() / TCO.abs().max())
    print(f'  {prefix}: the reference against itself with permuted unknowns: loss history {self_loss:.3g}, relative TCO {self_TCO:.3g}')
    assert max(self_loss, self_TCO) < SELF_CEILING, (prefix, 'the reference does not determine this scene to the ceiling', self_loss, self_TCO)
    out[prefix + 'self_loss'] = np.array(self_loss); out[prefix + 'self_TCO'] = np.array(self_TCO)
    out[prefix + 'obj_ids'] = np.array(problem.cand_obj_ids, np.int64); out[prefix + 'view_ids'] = np.array(problem.cand_view_ids, np.int64)
    out[prefix + 'visibility'] = problem.visibility_matrix.numpy()
    oi = problem.obj_infos
    out[prefix + 'objinfo_obj_id'] = oi['obj_id'].values.astype(np.int64); out[prefix + 'objinfo_n_cand'] = oi['n_cand'].values.astype(np.int64)
    out[prefix + 'objinfo_score'] = oi['score'].values.astype(np.float64)
    out[prefix + 'objinfo_label'] = np.array([int(l[4:]) - 1 for l in oi['label'].values], np.int64)
    out[prefix + 'objinfo_columns'] = np.array(list(oi.columns))
    keys = sorted(problem.v2v1_TC2C1_map)
    out[prefix + 'v2v1_keys'] = np.array(keys, np.int64)
    out[prefix + 'v2v1_TC2C1'] = torch.stack([problem.v2v1_TC2C1_map[k] for k in keys]).numpy()

    # alignment at the initial state: distances, the chosen symmetry, and its margin over the runner-up
    TWO_9d0, TCW_9d0 = h['TWO_9d'][0].detach(), h['TCW_9d'][0].detach()
    with torch.no_grad():
        dists, aligned = problem.align_TCO_cand(TWO_9d0, TCW_9d0)
        from cosypose.lib3d.transform_ops import compute_transform_from_pose9d
        TCO0 = compute_transform_from_pose9d(TCW_9d0)[problem.cand_view_ids] @ compute_transform_from_pose9d(TWO_9d0)[problem.cand_obj_ids]
        best = np.zeros(len(cand), np.int64)
        gap = np.inf
        for c in range(len(cand)):
            m = int(scene['cand_label_id'][c])
            pts = mesh_db.points[m][None]
            d = [float(R['sdist'].reprojected_dist(cand.poses[c][None] @ mesh_db.symmetries[m, k][None], TCO0[c][None],
                                                   problem.K[problem.cand_view_ids[c]][None], pts)) for k in range(int(scene['n_sym'][m]))]
            best[c] = int(np.argmin(d))
            assert (cand.poses[c] @ mesh_db.symmetries[m, best[c]] - aligned[c]).abs().max() < 1e-12
            if len(d) > 1:
                gap = min(gap, np.partition(d, 1)[1] - min(d))
    assert gap >= 1e-3, (prefix, 'best symmetry within 1e-3 px of the runner-up', gap)
    print(f'  {prefix}: best symmetry beats the runner-up by >= {gap:.3g} px; chosen {np.bincount(best).tolist()}')
    out[prefix + 'align_dists'] = dists.numpy(); out[prefix + 'align_sym'] = best; out[prefix + 'align_TCO'] = aligned.numpy()
    out[prefix + 'TWO_9d_init'] = TWO_9d0.numpy(); out[prefix + 'TCW_9d_init'] = TCW_9d0.numpy()
    out[prefix + 'TWO_9d_final'] = h['TWO_9d'][-1].detach().numpy(); out[prefix + 'TCW_9d_final'] = h['TCW_9d'][-1].detach().numpy()
    jac = {}
    if jacobian:
        for tag, (a, c) in dict(init=(TWO_9d0, TCW_9d0), final=(h['TWO_9d'][-1].detach(), h['TCW_9d'][-1].detach())).items():
            errors, loss, J_TWO, J_TCW = problem.forward_jacobian(a.clone(), c.clone(), 25)
            jac[f'{prefix}{tag}_errors'] = errors.detach().numpy(); jac[f'{prefix}{tag}_loss'] = np.array(float(loss))
            jac[f'{prefix}{tag}_J_TWO'] = compact_jacobian(J_TWO, np.array(problem.residuals_ids['obj_id']))
            jac[f'{prefix}{tag}_J_TCW'] = compact_jacobian(J_TCW, np.array(problem.residuals_ids['view_id']))
    return jac


def main():
    R = reference()
    out, jac = {}, {}
    for i, (seed, n_obj, n_views, P) in SCENES.items():
        print(f'scene {i}: seed {seed}, {n_obj} objects, {n_views} views, {P} points')
        jac.update(run_scene(R, syn.make_ba_scene(seed, n_obj, n_views, P), out, f's{i}_', i in JACOBIAN_SCENES))
    assert out['s4_n_rejected'] >= 1, 'scene 4 must also reject steps'
    for i in FIXED_CAMERA_SCENES:
        seed, n_obj, n_views, P = SCENES[i]
        print(f'scene {i}, exact view pairs, fixed cameras')
        run_scene(R, syn.make_ba_scene(seed, n_obj, n_views, P, exact_pairs=True), out, f'f{i}_', False, optimize_cameras=False, min_accept=5)
        assert (out[f'f{i}_hist_TCW_9d'] == out[f'f{i}_hist_TCW_9d'][0]).all()

    # make_view_groups: two components and a one-way edge (30 -> 31 only: 31 is a group of its own)
    import pandas as pd
    v1 = np.array([10, 11, 11, 12, 12, 10, 20, 21, 30, 30, 30], np.int64)
    v2 = np.array([11, 10, 12, 11, 10, 12, 21, 20, 31, 10, 10], np.int64)
    pairs = R['tc'].PandasTensorCollection(pd.DataFrame(dict(view1=v1, view2=v2)), TC1C2=torch.eye(4).repeat(len(v1), 1, 1))
    groups = R['ba'].make_view_groups(pairs)
    out['vg_view1'] = v1; out['vg_view2'] = v2
    out['vg_view_id'] = groups['view_id'].values.astype(np.int64); out['vg_view_group'] = groups['view_group'].values.astype(np.int64)
    assert len(set(out['vg_view_group'].tolist())) >= 3

    # symmetric_distance_reprojected in float32 on the inputs of reference_golden_dist.npz, with a K per item
    g = np.load(HERE / 'reference_golden_dist.npz')
    n_obj = g['sd_pts'].shape[0]
    labels_all = np.array([f'obj_{i:06d}' for i in range(1, n_obj + 1)])
    infos = {l: dict(label=l, n_points=g['sd_pts'].shape[1], n_sym=int(g['sd_nsym'][i])) for i, l in enumerate(labels_all)}
    mesh_db = R['BatchedMeshes'](infos, labels_all, torch.from_numpy(g['sd_pts']), torch.from_numpy(g['sd_sym'])).float()
    rs = np.random.RandomState(11)
    B = len(g['sd_obj'])
    K = np.tile(np.array([[600., 0, 320], [0, 600., 240], [0, 0, 1]], np.float32), (B, 1, 1))
    K[:, 0, 0] += rs.uniform(-40, 40, B).astype(np.float32); K[:, 1, 1] += rs.uniform(-40, 40, B).astype(np.float32)
    K[:, :2, 2] += rs.uniform(-15, 15, (B, 2)).astype(np.float32)
    with torch.no_grad():
        d, S12 = R['sdist'].symmetric_distance_reprojected(torch.from_numpy(g['sd_T1']), torch.from_numpy(g['sd_T2']), torch.from_numpy(K),
                                                           labels_all[g['sd_obj']], mesh_db)
    out['sdr_K'] = K; out['sdr_dists'] = d.numpy(); out['sdr_S12'] = S12.numpy()

    save_npz(HERE / 'reference_golden_ba.npz', out)
    save_npz(HERE / 'reference_golden_ba_jac.npz', jac)
    for f in ('reference_golden_ba.npz', 'reference_golden_ba_jac.npz'):
        print('wrote', f, (HERE / f).stat().st_size, 'bytes')


if __name__ == '__main__':
    main()
