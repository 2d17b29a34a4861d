"""Scene-level bundle adjustment (CosyPose stage 3), same surface as the reference's cosypose/multiview/bundle_adjustment.py:22-351.

`MultiviewRefinement.solve` moves the object poses TWO and the camera poses TCW (9-D states: ortho6d rotation + translation) by
Levenberg-Marquardt until the objects' mesh points reproject onto where the per-view candidates put them.  The reference replicates all
parameters once per residual, gets the Jacobian from autograd and inverts J^T J + lambda I on the CPU; here a linearisation is three
launches of libcosyhip.so (kernels_ba.hip: align, linearise, accumulate) that never form the dense Jacobian, and a step is one more
(Cholesky solve).  All of it computes in FLOAT64 whatever the inputs' dtype (they are widened once; DESIGN.md "Bundle adjustment" has
the measurements that made float32 unusable); poses come back in the candidates' dtype.

Host work: the constructor (id maps, visibility matrix, pair map: pandas / numpy, no device access), the initialisation walk over the
view graph (a few 4x4 products per view, float64 numpy), and the accept / reject logic of the loop, which reads ONE scalar -- the
loss -- back per linearisation.

`solve_problems` takes MANY problems through one set of launches: the batch is their concatenation (`_batch_plan`), the accept / reject /
stop logic runs on the device per problem (cosy_ba_batch_decide / cosy_ba_batch_record), and the host reads back only the number of
unfinished problems, once per `poll_every` iterations.  The kernels share their device code with the single-problem entries, so a
problem gets the same bits from both.
"""
import ctypes
import math
import time
from collections import defaultdict

import numpy as np
import pandas as pd
import torch

from . import tensor_collection as tc
from ._lib import lib, check, ptr, stream, require_device

MAX_BLOCKS = 128    # objects + views (kernels_ba.hip: n = 9 * blocks <= 1152)


class SamplerError(Exception):
    pass


def make_obj_infos(matched_candidates):
    """Per obj_id: first label, summed score, number of candidates (reference multiview/ransac.py:119-125)."""
    infos = matched_candidates.infos.loc[:, ['obj_id', 'score', 'label']]
    gb = infos.groupby('obj_id', sort=True)
    out = gb.agg(score=('score', 'sum'), label=('label', 'first'), n_cand=('score', 'size')).reset_index(drop=False)
    out['n_cand'] = out['n_cand'].astype(int)
    return out


def _strong_components(n, edges):
    """Strongly connected components of a directed graph on 0..n-1 (Tarjan, iterative).  -> (n,) component numbers."""
    adj = [[] for _ in range(n)]
    for a, b in edges:
        adj[a].append(b)
    index = [-1] * n
    low = [0] * n
    on_stack = [False] * n
    comp = [-1] * n
    stack = []
    counter = n_comp = 0
    for root in range(n):
        if index[root] >= 0:
            continue
        work = [(root, 0)]
        while work:
            v, i = work.pop()
            if i == 0:
                index[v] = low[v] = counter
                counter += 1
                stack.append(v)
                on_stack[v] = True
            descended = False
            while i < len(adj[v]):
                w = adj[v][i]
                i += 1
                if index[w] < 0:
                    work.append((v, i))
                    work.append((w, 0))
                    descended = True
                    break
                if on_stack[w]:
                    low[v] = min(low[v], index[w])
            if descended:
                continue
            if low[v] == index[v]:
                while True:
                    w = stack.pop()
                    on_stack[w] = False
                    comp[w] = n_comp
                    if w == v:
                        break
                n_comp += 1
            if work:
                u = work[-1][0]
                low[u] = min(low[u], low[v])
    return np.asarray(comp, dtype=np.int64)


def make_view_groups(pairs_TC1C2):
    """view_id -> view_group: strongly connected components of the directed graph view1 -> view2 (reference :22-35).  The group
    numbers are labels only (their order is not the reference's scipy numbering); the partition is the same."""
    v1 = np.asarray(pairs_TC1C2.infos['view1'].values)
    v2 = np.asarray(pairs_TC1C2.infos['view2'].values)
    views = np.unique(np.concatenate([v1, v2]))
    local = {v: n for n, v in enumerate(views)}
    comp = _strong_components(len(views), [(local[a], local[b]) for a, b in zip(v1, v2)])
    return pd.DataFrame(dict(view_id=views, view_group=comp))


def _invert_T_np(T):
    out = T.copy()
    Rt = np.swapaxes(T[..., :3, :3], -1, -2)
    out[..., :3, :3] = Rt
    out[..., :3, 3] = -(Rt @ T[..., :3, 3:])[..., 0]
    return out


def compute_transform_from_pose9d(pose9d):
    """(..., 9) -> (..., 4, 4), reference lib3d/transform_ops.py:54-64 / rotations.py:6-21 (plumbing for the outputs; the kernels have
    their own)."""
    x_raw, y_raw = pose9d[..., 0:3], pose9d[..., 3:6]
    x = x_raw / torch.norm(x_raw, p=2, dim=-1, keepdim=True)
    z = torch.cross(x, y_raw, dim=-1)
    z = z / torch.norm(z, p=2, dim=-1, keepdim=True)
    y = torch.cross(z, x, dim=-1)
    T = torch.zeros(*pose9d.shape[:-1], 4, 4, dtype=pose9d.dtype, device=pose9d.device)
    T[..., :3, :3] = torch.stack((x, y, z), -1)
    T[..., :3, 3] = pose9d[..., 6:]
    T[..., 3, 3] = 1
    return T


def invert_T(T):
    Rt = T[..., :3, :3].transpose(-2, -1)
    out = T.clone()
    out[..., :3, :3] = Rt
    out[..., :3, [-1]] = -Rt @ T[..., :3, [-1]]
    return out


class MultiviewRefinement:
    def __init__(self, candidates, cameras, pairs_TC1C2, mesh_db):
        if len(candidates) == 0:
            raise ValueError('MultiviewRefinement: no candidates')
        self.device, self.dtype = candidates.device, candidates.poses.dtype
        self.mesh_db = mesh_db

        view_ids = np.unique(candidates.infos['view_id'])
        cam_view_ids = np.asarray(cameras.infos['view_id'].values)
        missing = [v for v in view_ids if v not in set(cam_view_ids.tolist())]
        if missing:
            raise ValueError(f'MultiviewRefinement: candidates in views {missing} but `cameras` has no such view_id')
        keep = np.where(np.isin(cam_view_ids, view_ids))[0]
        cameras = cameras[keep]
        keep = np.where(np.logical_and(np.isin(pairs_TC1C2.infos['view1'], view_ids), np.isin(pairs_TC1C2.infos['view2'], view_ids)))[0]
        pairs_TC1C2 = pairs_TC1C2[keep]

        self.cam_infos = cameras.infos
        self.view_to_id = {view_id: n for n, view_id in enumerate(self.cam_infos['view_id'])}
        self.K = cameras.K.to(self.device).to(self.dtype)
        self.n_views = len(self.cam_infos)

        self.obj_infos = make_obj_infos(candidates)
        self.obj_to_id = {obj_id: n for n, obj_id in enumerate(self.obj_infos['obj_id'])}
        self.n_points = mesh_db.points.shape[1]
        self.n_objects = len(self.obj_infos)

        self.cand = candidates
        self.cand_TCO = candidates.poses
        self.cand_labels = candidates.infos['label']
        self.cand_view_ids = [self.view_to_id[view_id] for view_id in candidates.infos['view_id']]
        self.cand_obj_ids = [self.obj_to_id[obj_id] for obj_id in candidates.infos['obj_id']]
        self.n_candidates = len(self.cand_TCO)
        self.visibility_matrix = self.make_visibility_matrix(self.cand_view_ids, self.cand_obj_ids)

        # (view2, view1) -> row of the pair list: TC2C1 = inv(TC1C2[row]); later rows win, as in the reference's dict
        self.v2v1_pair_row = {(self.view_to_id[v2], self.view_to_id[v1]): n
                              for n, (v1, v2) in enumerate(zip(pairs_TC1C2.infos['view1'], pairs_TC1C2.infos['view2']))}
        self.ov_cand_row = {(o, v): n for n, (o, v) in enumerate(zip(self.cand_obj_ids, self.cand_view_ids))}
        self._pairs_TC1C2 = pairs_TC1C2.TC1C2
        self._host = None
        self._dev = None

    def make_visibility_matrix(self, cand_view_ids, cand_obj_ids):
        matrix = np.zeros((self.n_objects, self.n_views), dtype=np.int32)
        matrix[cand_obj_ids, cand_view_ids] = 1
        return torch.as_tensor(matrix).to(self.device)

    # ---- initialisation (host, float64) ----------------------------------------------------------------------------------
    def _host_state(self):
        if self._host is None:
            TC1C2 = self._pairs_TC1C2.detach().cpu().double().numpy().reshape(-1, 4, 4)
            self._host = dict(TC2C1=_invert_T_np(TC1C2), cand_TCO=self.cand_TCO.detach().cpu().double().numpy(),
                              visibility=self.visibility_matrix.cpu().numpy())
        return self._host

    def _sample_initial(self, seed):
        host = self._host_state()
        TWO = np.full((self.n_objects, 4, 4), np.nan)
        TWC = np.full((self.n_views, 4, 4), np.nan)
        object_to_views = defaultdict(set)
        for v in range(self.n_views):
            for o in range(self.n_objects):
                if host['visibility'][o, v]:
                    object_to_views[o].add(v)

        np_random = np.random.RandomState(seed)
        views_ordered = np_random.permutation(np.arange(self.n_views))
        objects_ordered = np_random.permutation(np.arange(self.n_objects))

        w = views_ordered[0]
        TWC[w] = np.eye(4)
        views_initialized = {w, }
        views_to_initialize = set(np.arange(self.n_views)) - views_initialized

        n_pass = 20
        n = 0
        while len(views_to_initialize) > 0:
            for v1 in views_ordered:
                if v1 in views_to_initialize:
                    for v2 in views_ordered:
                        if v2 not in views_initialized:
                            continue
                        if (v2, v1) in self.v2v1_pair_row:
                            TWC[v1] = TWC[v2] @ host['TC2C1'][self.v2v1_pair_row[(v2, v1)]]
                            views_to_initialize.remove(v1)
                            views_initialized.add(v1)
                            break
            n += 1
            if n >= n_pass:
                raise SamplerError('Cannot find an initialization')

        for o in objects_ordered:
            for v in views_ordered:
                if v in object_to_views[o]:
                    TWO[o] = TWC[v] @ host['cand_TCO'][self.ov_cand_row[(o, v)]]
                    break
        return TWO, TWC

    def sample_initial_TWO_TWC(self, seed):
        TWO, TWC = self._sample_initial(seed)
        return torch.as_tensor(TWO).to(self.device).to(self.dtype), torch.as_tensor(TWC).to(self.device).to(self.dtype)

    @staticmethod
    def extract_pose9d(T):
        return torch.cat((T[..., :3, :2].transpose(-1, -2).flatten(-2, -1), T[..., :3, -1]), dim=-1)

    # ---- device state ----------------------------------------------------------------------------------------------------
    def _device_state(self):
        if self._dev is not None:
            return self._dev
        mesh_db = self.mesh_db
        require_device(self.cand_TCO, self.K, mesh_db.points, mesh_db.symmetries)
        if self.n_objects + self.n_views > MAX_BLOCKS:
            raise ValueError(f'MultiviewRefinement: {self.n_objects} objects + {self.n_views} views > {MAX_BLOCKS}')
        dev, f64 = self.cand_TCO.device, torch.float64
        d = dict()
        d['cand_TCO'] = self.cand_TCO.detach().to(f64).contiguous()
        d['K'] = self.K.detach().to(dev).to(f64).contiguous()
        d['pts'] = mesh_db.points.detach().to(f64).contiguous()
        d['sym'] = mesh_db.symmetries.detach().to(f64).contiguous()
        n_mesh, P, S = d['pts'].shape[0], d['pts'].shape[1], d['sym'].shape[1]
        host_ids = [np.ascontiguousarray(a, dtype=np.int32) for a in (
            self.cand_obj_ids, self.cand_view_ids, [mesh_db.label_to_id[l] for l in self.cand_labels],
            [mesh_db.label_to_id[l] for l in self.obj_infos['label']])]
        n_sym = np.fromiter((mesh_db.infos[l]['n_sym'] for l in mesh_db.labels), dtype=np.int32, count=n_mesh)
        d['n_sym'] = torch.as_tensor(n_sym).to(dev)
        nc, no, nv = self.n_candidates, self.n_objects, self.n_views
        d['ids'] = torch.empty(3 * nc + no, dtype=torch.int32, device=dev)
        check(lib().cosy_ba_upload_ids(*(a.ctypes.data for a in host_ids), nc, no, nv, n_mesh, ptr(d['ids']), stream()))
        torch.cuda.current_stream().synchronize()       # the host arrays are read by the copies just queued
        n = 9 * (no + nv)
        d.update(n_mesh=n_mesh, P=P, S=S, n=n, n_res=2 * P * nc)
        d['ws'] = torch.empty(lib().cosy_ba_workspace_bytes(nc, P, no, nv), dtype=torch.uint8, device=dev)
        for name, shape in (('dists', (nc,)), ('aligned', (nc, 4, 4)), ('errors', (2 * P * nc,)), ('loss', (1,)), ('A', (n, n)), ('b', (n,)),
                            ('h', (n,))):
            d[name] = torch.empty(shape, dtype=f64, device=dev)
        d['best'] = torch.empty(nc, dtype=torch.int32, device=dev)
        self._dev = d
        return d

    def _state64(self, TWO_9d, TCW_9d):
        require_device(TWO_9d, TCW_9d)
        assert TWO_9d.shape == (self.n_objects, 9) and TCW_9d.shape == (self.n_views, 9)
        return TWO_9d.detach().to(torch.float64).contiguous(), TCW_9d.detach().to(torch.float64).contiguous()

    def _align(self, TWO_9d, TCW_9d):
        d = self._device_state()
        check(lib().cosy_ba_align(ptr(TWO_9d), ptr(TCW_9d), ptr(d['cand_TCO']), ptr(d['K']), ptr(d['ids']), ptr(d['pts']), ptr(d['sym']),
                                  ptr(d['n_sym']), self.n_candidates, self.n_objects, self.n_views, d['n_mesh'], d['P'], d['S'],
                                  ptr(d['dists']), ptr(d['best']), ptr(d['aligned']), stream()))

    def _linearize(self, TWO_9d, TCW_9d, residuals_threshold, J_obj=None, J_view=None):
        """align + linearise at a float64 state: fills the errors, loss, A, b buffers (4 launches, nothing read back)."""
        d = self._device_state()
        self._align(TWO_9d, TCW_9d)
        check(lib().cosy_ba_linearize(ptr(TWO_9d), ptr(TCW_9d), ptr(d['aligned']), ptr(d['K']), ptr(d['ids']), ptr(d['pts']),
                                      self.n_candidates, self.n_objects, self.n_views, d['n_mesh'], d['P'], float(residuals_threshold),
                                      ptr(d['errors']), ptr(d['loss']), ptr(d['A']), ptr(d['b']), ptr(J_obj), ptr(J_view), ptr(d['ws']),
                                      stream()))

    def _solve(self, lambd):
        d = self._device_state()
        check(lib().cosy_ba_solve(ptr(d['A']), ptr(d['b']), d['n'], float(lambd), ptr(d['h']), ptr(d['ws']), stream()))
        return d['h']

    # ---- the reference's methods -------------------------------------------------------------------------------------------
    def align_TCO_cand(self, TWO_9d, TCW_9d):
        """-> (dists (n_cand) in pixels, TCO_cand_aligned (n_cand,4,4) = cand_TCO @ best symmetry), float64."""
        d = self._device_state()
        self._align(*self._state64(TWO_9d, TCW_9d))
        return d['dists'].clone(), d['aligned'].clone()

    def forward_jacobian(self, TWO_9d, TCW_9d, residuals_threshold):
        """-> errors (n_res), loss (0-d), J_TWO (n_res, 9), J_TCW (n_res, 9), float64 on the device: the Jacobian of the reprojection of
        residual r with respect to ITS object's and ITS view's 9 parameters (all other entries of the reference's dense
        (n_res, n_objects, 9) / (n_res, n_views, 9) gradients are zero)."""
        d = self._device_state()
        J_obj = torch.empty(d['n_res'], 9, dtype=torch.float64, device=d['A'].device)
        J_view = torch.empty_like(J_obj)
        self._linearize(*self._state64(TWO_9d, TCW_9d), residuals_threshold, J_obj, J_view)
        return d['errors'].clone(), d['loss'][0].clone(), J_obj, J_view

    def normal_equations(self, TWO_9d, TCW_9d, residuals_threshold):
        """-> A = J^T J (n, n), b = J^T e (n) at a state, n = 9 (n_objects + n_views), objects first; float64."""
        d = self._device_state()
        self._linearize(*self._state64(TWO_9d, TCW_9d), residuals_threshold)
        return d['A'].clone(), d['b'].clone()

    def optimize_lm(self, TWO_9d, TCW_9d, optimize_cameras=True, n_iterations=50, residuals_threshold=25, lambd0=1e-3, L_down=9, L_up=11,
                    eps=1e-5):
        # See http://people.duke.edu/~hpgavin/ce281/lm.pdf; control flow of the reference (:238-277) line for line.
        # history['loss'] holds 0-d float64 device tensors, as the reference's; the decisions use the one scalar read back per
        # linearisation.  TWO_9d / TCW_9d: float64 on the device.
        d = self._device_state()
        TWO_9d, TCW_9d = self._state64(TWO_9d, TCW_9d)
        n_params_TWO = TWO_9d.numel()

        self.n_linearisations = 0

        def linearize(a, c):
            self._linearize(a, c, residuals_threshold)
            self.n_linearisations += 1
            return d['loss'][0].clone(), d['loss'].item()

        prev_iter_is_update = False
        lambd = lambd0
        done = False
        history = defaultdict(list)
        for n in range(n_iterations):

            if not prev_iter_is_update:
                loss, loss_value = linearize(TWO_9d, TCW_9d)

            history['TWO_9d'].append(TWO_9d)
            history['TCW_9d'].append(TCW_9d)
            history['loss'].append(loss)
            history['lambda'].append(lambd)
            history['iteration'].append(n)

            if done:
                break

            h = self._solve(lambd)       # the JOINT step; with fixed cameras its camera part is dropped
            TWO_9d_updated = TWO_9d + h[:n_params_TWO].view(self.n_objects, 9)
            if optimize_cameras:
                TCW_9d_updated = TCW_9d + h[n_params_TWO:].view(self.n_views, 9)
            else:
                TCW_9d_updated = TCW_9d

            next_loss, next_loss_value = linearize(TWO_9d_updated, TCW_9d_updated)

            rho = loss_value - next_loss_value
            if abs(rho) < eps:
                done = True
            elif rho > eps:
                TWO_9d = TWO_9d_updated
                TCW_9d = TCW_9d_updated
                loss, loss_value = next_loss, next_loss_value
                lambd = max(lambd / L_down, 1e-7)
                prev_iter_is_update = True
            else:
                lambd = min(lambd * L_up, 1e7)
                prev_iter_is_update = False
        return TWO_9d, TCW_9d, history

    def robust_initialization_TWO_TCW(self, n_init=1):
        d = self._device_state()
        TWO_9d_init, TCW_9d_init, dists = [], [], []
        for n in range(n_init):
            TWO, TWC = self._sample_initial(n)
            dev = d['A'].device
            TWO_9d = self.extract_pose9d(torch.as_tensor(TWO).to(dev)).contiguous()
            TCW_9d = self.extract_pose9d(torch.as_tensor(_invert_T_np(TWC)).to(dev)).contiguous()
            self._align(TWO_9d, TCW_9d)
            TWO_9d_init.append(TWO_9d)
            TCW_9d_init.append(TCW_9d)
            dists.append(d['dists'].mean())
        best_iter = int(torch.stack(dists).argmin()) if n_init > 1 else 0
        return TWO_9d_init[best_iter], TCW_9d_init[best_iter]

    def _scene_infos_batch(self, states):
        """[(TWO_9d, TCW_9d), ...] -> [(objects, cameras), ...] through ONE batched conversion: equal states give equal bits whichever
        list position they have (torch picks its kernels by the batch shape)."""
        TWO = compute_transform_from_pose9d(torch.stack([a for a, _ in states])).to(self.dtype)
        TWC = invert_T(compute_transform_from_pose9d(torch.stack([c for _, c in states]))).to(self.dtype)
        return [(tc.PandasTensorCollection(infos=self.obj_infos, TWO=TWO[n]), tc.PandasTensorCollection(infos=self.cam_infos, TWC=TWC[n], K=self.K))
                for n in range(len(states))]

    def make_scene_infos(self, TWO_9d, TCW_9d):
        return self._scene_infos_batch([(TWO_9d, TCW_9d)])[0]

    def convert_history(self, history, also=()):
        """Adds `objects` / `cameras` of every history entry; -> (history, the same for the extra states `also`), all of them converted
        in one batch."""
        states = list(zip(history['TWO_9d'], history['TCW_9d'])) + list(also)
        converted = self._scene_infos_batch(states) if states else []
        n = len(history['iteration'])
        history['objects'] = [o for o, _ in converted[:n]]
        history['cameras'] = [c for _, c in converted[:n]]
        return history, converted[n:]

    def solve(self, sample_n_init=1, **lm_kwargs):
        t0 = time.time()
        TWO_9d_init, TCW_9d_init = self.robust_initialization_TWO_TCW(n_init=sample_n_init)
        torch.cuda.synchronize()
        t1 = time.time()
        TWO_9d_opt, TCW_9d_opt, history = self.optimize_lm(TWO_9d_init, TCW_9d_init, **lm_kwargs)
        torch.cuda.synchronize()
        t2 = time.time()
        history, ((objects, cameras), (objects_init, cameras_init)) = self.convert_history(
            history, also=[(TWO_9d_opt, TCW_9d_opt), (TWO_9d_init, TCW_9d_init)])
        torch.cuda.synchronize()
        t3 = time.time()
        return dict(objects_init=objects_init, cameras_init=cameras_init, objects=objects, cameras=cameras, history=history,
                    time_init=t1 - t0, time_opt=t2 - t1, time_misc=t3 - t2)


# ---- many problems per call ------------------------------------------------------------------------------------------------------
def _batch_plan(problems):
    """The id and offset tables of a batch = the concatenation of `problems`, as numpy arrays (no device is touched, so CPU-tensor
    problems do).  Candidates carry GLOBAL object and view rows: cand_obj[c] = obj_off[g] + the problem's own object id, cand_view[c]
    = view_off[g] + its view id; cand_mesh / obj_mesh are rows of the shared mesh table.  cand_off, obj_off, view_off, par_off (9 x
    blocks) and A_off (n_g^2) are exclusive prefix sums with G + 1 entries; n = 9 (objects + views) per problem.  Raises ValueError for
    problems that do not share one mesh_db (the same `points` and `symmetries` tensors) and for one over MAX_BLOCKS."""
    problems = list(problems)
    if not problems:
        raise ValueError('_batch_plan: no problems')
    mesh_db = problems[0].mesh_db
    for g, p in enumerate(problems):
        if p.mesh_db is not mesh_db and (p.mesh_db.points is not mesh_db.points or p.mesh_db.symmetries is not mesh_db.symmetries):
            raise ValueError(f'solve_problems: problem {g} has another mesh_db than problem 0 (a batch shares one points / symmetries table)')
        if p.n_objects + p.n_views > MAX_BLOCKS:
            raise ValueError(f'solve_problems: problem {g}: {p.n_objects} objects + {p.n_views} views > {MAX_BLOCKS}')
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    prefix = lambda sizes: np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))])
    cand_off, obj_off, view_off = (prefix([getattr(p, k) for p in problems]) for k in ('n_candidates', 'n_objects', 'n_views'))
    blocks = np.asarray([p.n_objects + p.n_views for p in problems], dtype=np.int64)
    l2i = mesh_db.label_to_id
    return dict(
        G=len(problems), n=9 * blocks, max_blocks=int(blocks.max()),
        cand_obj=i32(np.concatenate([np.asarray(p.cand_obj_ids, dtype=np.int64) + obj_off[g] for g, p in enumerate(problems)])),
        cand_view=i32(np.concatenate([np.asarray(p.cand_view_ids, dtype=np.int64) + view_off[g] for g, p in enumerate(problems)])),
        cand_mesh=i32([l2i[l] for p in problems for l in p.cand_labels]),
        obj_mesh=i32([l2i[l] for p in problems for l in p.obj_infos['label']]),
        cand_off=i32(cand_off), obj_off=i32(obj_off), view_off=i32(view_off), par_off=9 * prefix(blocks), A_off=prefix((9 * blocks) ** 2))


def _pose9d_np(T):
    """MultiviewRefinement.extract_pose9d on numpy: copies only"""
    return np.concatenate([np.swapaxes(T[..., :3, :2], -1, -2).reshape(*T.shape[:-2], 6), T[..., :3, 3]], axis=-1)


class _Batch:
    """The device side of one solve_problems call: tables, states, control records, history rows, workspace."""

    def __init__(self, problems, plan, TWO_9d, TCW_9d, optimize_cameras, n_iterations, residuals_threshold, lambd0, L_down, L_up, eps,
                 history):
        from ._lib import BaBatch, BaCtrl
        mesh_db = problems[0].mesh_db
        f64 = torch.float64
        cand_TCO = torch.cat([p.cand_TCO.detach() for p in problems]).to(f64).contiguous()
        K = torch.cat([p.K.detach() for p in problems]).to(f64).contiguous()
        pts = mesh_db.points.detach().to(f64).contiguous()
        sym = mesh_db.symmetries.detach().to(f64).contiguous()
        require_device(cand_TCO, K, pts, sym, TWO_9d, TCW_9d)
        dev = cand_TCO.device
        G, nc, no, nv = plan['G'], len(plan['cand_obj']), len(plan['obj_mesh']), int(plan['view_off'][-1])
        n_mesh = pts.shape[0]
        n_sym = torch.as_tensor(np.fromiter((mesh_db.infos[l]['n_sym'] for l in mesh_db.labels), dtype=np.int32, count=n_mesh)).to(dev)
        table = torch.empty(lib().cosy_ba_batch_table_bytes(G, nc, no), dtype=torch.uint8, device=dev)
        a_total, max_blocks = ctypes.c_longlong(0), ctypes.c_int(0)
        check(lib().cosy_ba_batch_upload(*(plan[k].ctypes.data for k in ('cand_obj', 'cand_view', 'cand_mesh', 'obj_mesh', 'cand_off', 'obj_off',
                                                                         'view_off')),
                                         G, n_mesh, ptr(table), ctypes.byref(a_total), ctypes.byref(max_blocks), stream()))
        assert a_total.value == int(plan['A_off'][-1]) and max_blocks.value == plan['max_blocks']
        ctrl = np.zeros(G, dtype=np.dtype(BaCtrl))
        ctrl['lambd'] = lambd0
        self.ctrl = torch.from_numpy(ctrl.view(np.uint8).reshape(G, -1)).to(dev)
        self.ctrl_dtype = ctrl.dtype
        rows = n_iterations
        self.TWO, self.TCW = TWO_9d.to(f64).contiguous().clone(), TCW_9d.to(f64).contiguous().clone()
        self.TWO_updated, self.TCW_updated = torch.empty_like(self.TWO), torch.empty_like(self.TCW)
        self.hist_iteration = torch.empty(G, rows, dtype=torch.int32, device=dev)
        self.hist_lambda = torch.empty(G, rows, dtype=f64, device=dev)
        self.hist_loss = torch.empty(G, rows, dtype=f64, device=dev)
        self.hist_TWO = torch.empty(rows, no, 9, dtype=f64, device=dev) if history else None
        self.hist_TCW = torch.empty(rows, nv, 9, dtype=f64, device=dev) if history else None
        self.ws = torch.empty(lib().cosy_ba_batch_workspace_bytes(nc, no + nv, a_total.value), dtype=torch.uint8, device=dev)
        self._keep = (table, cand_TCO, K, pts, sym, n_sym)
        self.c = BaBatch(G=G, n_cand=nc, n_obj=no, n_views=nv, n_mesh=n_mesh, P=pts.shape[1], S=sym.shape[1], max_blocks=max_blocks.value,
                         n_hist_rows=rows, optimize_cameras=int(bool(optimize_cameras)), a_total=a_total.value,
                         residuals_threshold=float(residuals_threshold), L_down=float(L_down), L_up=float(L_up), eps=float(eps),
                         table=ptr(table), cand_TCO=ptr(cand_TCO), K=ptr(K), pts_table=ptr(pts), sym_table=ptr(sym), n_sym=ptr(n_sym),
                         TWO_9d=ptr(self.TWO), TCW_9d=ptr(self.TCW), TWO_9d_updated=ptr(self.TWO_updated),
                         TCW_9d_updated=ptr(self.TCW_updated), ctrl=ptr(self.ctrl), hist_iteration=ptr(self.hist_iteration),
                         hist_lambda=ptr(self.hist_lambda), hist_loss=ptr(self.hist_loss), hist_TWO_9d=ptr(self.hist_TWO),
                         hist_TCW_9d=ptr(self.hist_TCW), workspace=ptr(self.ws))

    def iterate(self, n_first, n_count):
        check(lib().cosy_ba_batch_iterate(ctypes.addressof(self.c), n_first, n_count, stream()))

    def n_unfinished(self):
        """ONE host read: how many problems have not met their stop rule"""
        finished = self.ctrl.view(torch.int32)[:, self.ctrl_dtype.fields['finished'][1] // 4]
        return int((finished == 0).sum().item())


def solve_problems(problems, sample_n_init=1, optimize_cameras=True, n_iterations=50, residuals_threshold=25, lambd0=1e-3, L_down=9,
                   L_up=11, eps=1e-5, history=True, poll_every=8):
    """`MultiviewRefinement.solve` of every problem of `problems`, all of them advancing through the same launches -> one dict per
    problem with solve's keys objects_init, cameras_init, objects, cameras, history, and TWO_9d / TCW_9d: the final float64 states.
    history holds `iteration` (ints), `lambda` (floats) and `loss` (0-d float64 device tensors) and, with history=True, the states
    `TWO_9d` / `TCW_9d` of every entry; the per-entry `objects` / `cameras` collections are not built (problem.convert_history adds
    them).  A problem gets the same bits as from its own `solve`, whatever else is in the batch.

    The problems must share one mesh_db (ValueError otherwise, before any launch).  The initial states come from each problem's host
    walk (with sample_n_init > 1 each problem picks its best start on the device first, as solve does).  The host launches
    `poll_every` iterations at a time and then reads ONE number back, how many problems are still running, to stop early; one more
    read at the end fetches the history's lengths, lambdas and iteration numbers.  Batch-level figures go on the FIRST dict: `n_host_reads`,
    `n_iterations_launched`, `time_init`, `time_opt`, `time_misc` (seconds, as solve's, for the whole batch)."""
    problems = list(problems)
    if not problems:
        return []
    if n_iterations < 1 or poll_every < 1 or not lambd0 > 0:
        raise ValueError(f'solve_problems: n_iterations={n_iterations} poll_every={poll_every} lambd0={lambd0}')
    t0 = time.time()
    plan = _batch_plan(problems)                      # refuses mixed mesh tables and oversized problems before any launch
    require_device(*(p.cand_TCO for p in problems), problems[0].mesh_db.points, problems[0].mesh_db.symmetries)
    dev = problems[0].cand_TCO.device
    if sample_n_init == 1:
        starts = [p._sample_initial(0) for p in problems]
        TWO_9d_init = torch.as_tensor(np.concatenate([_pose9d_np(TWO) for TWO, _ in starts])).to(dev)
        TCW_9d_init = torch.as_tensor(np.concatenate([_pose9d_np(_invert_T_np(TWC)) for _, TWC in starts])).to(dev)
    else:
        starts = [p.robust_initialization_TWO_TCW(n_init=sample_n_init) for p in problems]
        TWO_9d_init, TCW_9d_init = torch.cat([a for a, _ in starts]), torch.cat([c for _, c in starts])
    batch = _Batch(problems, plan, TWO_9d_init, TCW_9d_init, optimize_cameras, n_iterations, residuals_threshold, lambd0, L_down, L_up, eps,
                   history)
    torch.cuda.synchronize()
    t1 = time.time()

    n_host_reads, n = 0, 0
    while n < n_iterations:
        count = min(poll_every, n_iterations - n)
        batch.iterate(n, count)
        n += count
        if n < n_iterations:
            n_host_reads += 1
            if batch.n_unfinished() == 0:
                break
    # the last read: the records (history lengths) and the small history columns
    n_hist = batch.ctrl.cpu().numpy().view(batch.ctrl_dtype)['n_hist'].ravel()
    host_iteration, host_lambda = batch.hist_iteration.cpu().numpy(), batch.hist_lambda.cpu().numpy()
    n_host_reads += 1
    t2 = time.time()

    # 4x4 outputs of all problems: one batched conversion of [final | initial] states
    TWO = compute_transform_from_pose9d(torch.stack([batch.TWO, TWO_9d_init]))
    TWC = invert_T(compute_transform_from_pose9d(torch.stack([batch.TCW, TCW_9d_init])))
    outs = []
    for g, p in enumerate(problems):
        o0, o1, v0, v1, k = plan['obj_off'][g], plan['obj_off'][g + 1], plan['view_off'][g], plan['view_off'][g + 1], int(n_hist[g])
        hist = {'iteration': host_iteration[g, :k].tolist(), 'lambda': host_lambda[g, :k].tolist(),
                'loss': list(batch.hist_loss[g, :k].unbind(0))}
        if history:
            hist['TWO_9d'] = list(batch.hist_TWO[:k, o0:o1].unbind(0))
            hist['TCW_9d'] = list(batch.hist_TCW[:k, v0:v1].unbind(0))
        TWO_p, TWC_p = TWO[:, o0:o1].to(p.dtype), TWC[:, v0:v1].to(p.dtype)
        outs.append(dict(objects_init=tc.PandasTensorCollection(infos=p.obj_infos, TWO=TWO_p[1]),
                         cameras_init=tc.PandasTensorCollection(infos=p.cam_infos, TWC=TWC_p[1], K=p.K),
                         objects=tc.PandasTensorCollection(infos=p.obj_infos, TWO=TWO_p[0]),
                         cameras=tc.PandasTensorCollection(infos=p.cam_infos, TWC=TWC_p[0], K=p.K), history=hist,
                         TWO_9d=batch.TWO[o0:o1], TCW_9d=batch.TCW[v0:v1]))
    torch.cuda.synchronize()
    t3 = time.time()
    outs[0].update(n_host_reads=n_host_reads, n_iterations_launched=n, time_init=t1 - t0, time_opt=t2 - t1, time_misc=t3 - t2)
    return outs
