"""A plain float64 restatement of what csrc/kernels_ba.hip computes, for tests/test_ba_kernels.py and test_bundle_adjustment.py.

CPU, torch / numpy float64 only, nothing imported from cosypose_amd.bundle_adjustment: pose9d -> T, K T p, the perspective division,
and the Jacobian of the reprojections from torch.autograd.functional.jacobian per candidate over its 18 parameters -- no analytic
chain rule, so it shares nothing with the kernel's derivation.  tests/test_bundle_adjustment_host.py pins it to the reference's stored
autograd runs (reference_golden_ba_jac.npz) on the CPU.
"""
import numpy as np
import torch

F64 = torch.float64


def t64(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float64))


def pose9d_to_T(a):
    """(..., 9) -> (..., 4, 4): R = [x y z] columns from ortho6d (x = a1/|a1|, z = x X a2 normalised, y = z X x), t = a[6:9]"""
    a1, a2, t = a[..., 0:3], a[..., 3:6], a[..., 6:9]
    x = a1 / a1.norm(dim=-1, keepdim=True)
    z = torch.linalg.cross(x, a2, dim=-1)
    z = z / z.norm(dim=-1, keepdim=True)
    y = torch.linalg.cross(z, x, dim=-1)
    top = torch.cat((torch.stack((x, y, z), -1), t[..., None]), -1)
    bottom = torch.zeros_like(top[..., :1, :])
    bottom[..., 0, 3] = 1
    return torch.cat((top, bottom), -2)


def project(K, T, p):
    """K (..., 3, 3), T (..., 4, 4), p (..., P, 3) -> pixels (..., P, 2); no z clamp"""
    ph = torch.cat((p, torch.ones_like(p[..., :1])), -1)
    s = ph @ (K @ T[..., :3, :]).transpose(-1, -2)
    return s[..., :2] / s[..., 2:]


def symmetry_distances(T1, T2, K, pts, sym, ns):
    """Over a batch of B items: mean over the points of |project(K, T1 S_k, p) - project(K, T2, p)| for every symmetry k.
    T1, T2 (B,4,4), K (B,3,3), pts (B,P,3), sym (B,S,4,4), ns (B,) symmetries that count (already clamped to S).
    -> dists (B,S) numpy (inf at k >= ns; all NaN where ns <= 0), best (B,) (first minimum wins; -1 where ns <= 0), margin (B,) of the
    best to the runner-up (inf with one symmetry)."""
    B, S = sym.shape[:2]
    uv1 = project(K[:, None], T1[:, None] @ sym, pts[:, None])          # (B,S,P,2)
    uv2 = project(K, T2, pts)[:, None]
    d = (uv1 - uv2).norm(dim=-1).mean(dim=-1).numpy().copy()            # (B,S)
    ns = np.asarray(ns)
    d[np.arange(S)[None] >= ns[:, None]] = np.inf
    best = d.argmin(axis=1)                                             # numpy: the first occurrence of the minimum
    srt = np.sort(d, axis=1)
    margin = srt[:, 1] - srt[:, 0] if S > 1 else np.full(B, np.inf)
    none = ns <= 0
    d[none] = np.nan
    best[none] = -1
    margin[none] = np.nan
    return d, best, margin


def reference(TWO_9d, TCW_9d, cand_TCO, K, cand_obj, cand_view, cand_mesh, obj_mesh, pts, sym, n_sym, threshold, jacobian=True):
    """The linearisation of the bundle adjustment at a state.  TWO_9d (n_obj,9), TCW_9d (n_views,9), cand_TCO (n_cand,4,4),
    K (n_views,3,3), the id arrays, pts (n_mesh,P,3), sym (n_mesh,S,4,4), n_sym (n_mesh).  Align reads the mesh of the CANDIDATE
    (cand_mesh), the residuals the mesh of its OBJECT (obj_mesh[cand_obj]).  -> dict of numpy float64:
      dists (n_cand,S), best, margin, aligned (n_cand,4,4) = cand_TCO @ S_best
      errors (n_cand * 2P) in the order (candidate, point, x|y), pix_scale = max |pixel coordinate| they are differences of, loss
      with jacobian=True also J_TWO, J_TCW (rows, 9), the dense J (rows, 9 (n_obj + n_views)), objects first, A = J^T J, b = J^T e,
      the un-cancelled scales A_scale = |J|^T |J| and b_scale = |J|^T |e|, and terms = 2P x the most candidates summed into one block."""
    TWO_9d, TCW_9d, cand_TCO, K, pts, sym = (t64(a) for a in (TWO_9d, TCW_9d, cand_TCO, K, pts, sym))
    cand_obj, cand_view, cand_mesh, obj_mesh = (np.asarray(a, dtype=np.int64) for a in (cand_obj, cand_view, cand_mesh, obj_mesh))
    n_cand, n_obj, n_views, P, S = len(cand_obj), len(TWO_9d), len(TCW_9d), pts.shape[1], sym.shape[1]
    TCO = pose9d_to_T(TCW_9d)[cand_view] @ pose9d_to_T(TWO_9d)[cand_obj]
    Kc = K[cand_view]
    ns = np.minimum(np.asarray(n_sym, dtype=np.int64)[cand_mesh], S)
    dists, best, margin = symmetry_distances(cand_TCO, TCO, Kc, pts[cand_mesh], sym[cand_mesh], ns)
    aligned = cand_TCO @ sym[cand_mesh, np.maximum(best, 0)]
    aligned[torch.as_tensor(best < 0)] = float('nan')
    p_obj = pts[obj_mesh[cand_obj]]
    y = project(Kc, aligned, p_obj)
    yhat = project(Kc, TCO, p_obj)
    errors = (y - yhat).reshape(-1)
    loss = torch.minimum(errors ** 2, torch.tensor(float(threshold), dtype=F64)).mean()
    out = dict(dists=dists, best=best, margin=margin, aligned=aligned.numpy(), errors=errors.numpy(), loss=float(loss),
               pix_scale=float(torch.maximum(y.abs().max(), yhat.abs().max())))
    if not jacobian:
        return out
    n_res, n = n_cand * 2 * P, 9 * (n_obj + n_views)
    J_TWO, J_TCW = torch.empty(n_res, 9, dtype=F64), torch.empty(n_res, 9, dtype=F64)
    for c in range(n_cand):
        def reprojection(x):
            return project(Kc[c], pose9d_to_T(x[9:]) @ pose9d_to_T(x[:9]), p_obj[c]).reshape(-1)
        Jc = torch.autograd.functional.jacobian(reprojection, torch.cat((TWO_9d[cand_obj[c]], TCW_9d[cand_view[c]])), vectorize=True)
        J_TWO[c * 2 * P:(c + 1) * 2 * P], J_TCW[c * 2 * P:(c + 1) * 2 * P] = Jc[:, :9], Jc[:, 9:]
    J = torch.zeros(n_res, n, dtype=F64)
    rows = torch.arange(n_res)[:, None]
    nine = torch.arange(9)[None]
    J[rows, torch.as_tensor(np.repeat(cand_obj, 2 * P))[:, None] * 9 + nine] = J_TWO
    J[rows, (n_obj + torch.as_tensor(np.repeat(cand_view, 2 * P)))[:, None] * 9 + nine] = J_TCW
    per_block = max(np.bincount(cand_obj, minlength=n_obj).max(), np.bincount(cand_view, minlength=n_views).max())
    out.update(J_TWO=J_TWO.numpy(), J_TCW=J_TCW.numpy(), J=J.numpy(), A=(J.t() @ J).numpy(), b=(J.t() @ errors).numpy(),
               A_scale=(J.abs().t() @ J.abs()).numpy(), b_scale=(J.abs().t() @ errors.abs()).numpy(), terms=int(2 * P * per_block))
    return out


def reprojected_distance_float32(T1, T2, K, obj_id, pts, sym, n_sym):
    """cosy_symmetric_distance_reprojected's formula evaluated in float64 on its float32 inputs, widened.  T1, T2 (B,4,4), K (B,3,3),
    obj_id (B,) or None (item b reads table row b), pts (n_obj,P,3), sym (n_obj,S,4,4), n_sym (n_obj,) or None (all S count).
    -> dists (B,S), best (B,), margin (B,), S12 (B,4,4) float32: the chosen rows of `sym` as they are."""
    for a in (T1, T2, K, pts, sym):
        assert np.asarray(a).dtype == np.float32
    B, S = len(T1), sym.shape[1]
    obj = np.arange(B) if obj_id is None else np.asarray(obj_id, dtype=np.int64)
    ns = np.full(B, S) if n_sym is None else np.minimum(np.asarray(n_sym, dtype=np.int64)[obj], S)
    dists, best, margin = symmetry_distances(t64(T1), t64(T2), t64(K), t64(pts)[obj], t64(sym)[obj], ns)
    return dists, best, margin, np.asarray(sym)[obj, best]


# ---- synthetic.make_ba_scene dicts ---------------------------------------------------------------------------------------------------
def scene_ids(scene):
    """cand_obj, cand_view, cand_mesh, obj_mesh of a make_ba_scene dict: views in the cameras' order, objects by ascending obj_id,
    an object's mesh that of its first candidate."""
    cand_view = np.array([np.flatnonzero(scene['cam_view_id'] == v)[0] for v in scene['cand_view_id']])
    obj_ids, first, cand_obj = np.unique(scene['cand_obj_id'], return_index=True, return_inverse=True)
    cand_mesh = np.asarray(scene['cand_label_id'], dtype=np.int64)
    return cand_obj.reshape(-1), cand_view, cand_mesh, cand_mesh[first]


def pose9d_of(T):
    """(..., 4, 4) numpy -> (..., 9): the first two columns of R, then t"""
    return np.concatenate((T[..., :3, 0], T[..., :3, 1], T[..., :3, 3]), axis=-1)


def state_from_candidates(scene, seed, sigma=3e-3):
    """A state derived from the candidates -- TWC the scene's cameras, TWO[o] = TWC[v] cand_TCO[c] of the object's first candidate --
    with N(0, sigma) added to every entry of the 9-D states, so that the residuals are of the order of pixels (without it a scene of
    one object and one view has e == 0 exactly).  -> TWO_9d (n_obj, 9), TCW_9d (n_views, 9), float64 numpy."""
    cand_obj, cand_view, _, _ = scene_ids(scene)
    first = np.array([np.flatnonzero(cand_obj == o)[0] for o in range(cand_obj.max() + 1)])
    TWC = np.asarray(scene['cam_TWC'], dtype=np.float64)
    TWO = TWC[cand_view[first]] @ scene['cand_poses'][first]
    rs = np.random.RandomState(seed)
    TWO_9d, TCW_9d = pose9d_of(TWO), pose9d_of(np.linalg.inv(TWC))
    return TWO_9d + sigma * rs.randn(*TWO_9d.shape), TCW_9d + sigma * rs.randn(*TCW_9d.shape)


def reference_of_scene(scene, TWO_9d, TCW_9d, threshold, jacobian=True):
    return reference(TWO_9d, TCW_9d, scene['cand_poses'], scene['cam_K'], *scene_ids(scene), scene['pts'], scene['sym'], scene['n_sym'],
                     threshold, jacobian=jacobian)
