"""Batched mesh database: the `mesh_db` object PosePredictor consumes.

Same surface as the reference's BatchedMeshes / Meshes
(cosypose/lib3d/rigid_mesh_database.py:59-94): `select(labels)` ->
`.sample_points(n, deterministic=True)`, `.points`, `.symmetries`, `.labels`,
`.label_to_id`, `.infos`, `.n_sym_mapping`.

MI355X-first addition: the 2000 point ids drawn by
sample_points(2000, deterministic=True) are the same for every call and every object
(np.random.RandomState(0).choice(Nmax, 2000, replace=False), cosypose/lib3d/mesh_ops.py:31-41),
so the sub-sampled table (n_obj, 2000, 3) is built ONCE on the device (`point_table`)
and kernels index it by object id instead of gathering B x Nmax x 3 floats per iteration.

MeshDataBase builds a BatchedMeshes from vertex arrays the caller holds (the reference's class, rigid_mesh_database.py:11-56, without
trimesh): `.batched()` reproduces the reference's bytes, and `from_models_info` fills in diameters the BOP files lack with
model_info (csrc/kernels_models.hip).  Loading meshes from .ply (MeshDataBase.from_object_ds) and resample_n_points
(trimesh.sample.sample_surface) need trimesh and stay out.
"""
from copy import deepcopy

import numpy as np
import torch

from .tensor_collection import TensorCollection


def deterministic_point_ids(n_max, n_points):
    return np.random.RandomState(0).choice(n_max, size=n_points, replace=False)


def sample_points(points, n_points, deterministic=False):
    assert points.dim() == 3
    assert n_points <= points.shape[1]
    rng = np.random.RandomState(0) if deterministic else np.random
    from ._lib import host_to_device
    ids = host_to_device(rng.choice(points.shape[1], size=n_points, replace=False), points.device)      # no wait for the queued kernels
    return torch.index_select(points, 1, ids)


class Meshes(TensorCollection):
    def __init__(self, infos, labels, points, symmetries):
        super().__init__()
        self.infos = infos
        self.labels = np.asarray(labels)
        self.register_tensor('points', points)
        self.register_tensor('symmetries', symmetries)

    def select_labels(self, labels):
        raise NotImplementedError

    def sample_points(self, n_points, deterministic=False):
        return sample_points(self.points, n_points, deterministic=deterministic)


class BatchedMeshes(TensorCollection):
    def __init__(self, infos, labels, points, symmetries):
        super().__init__()
        self.infos = infos
        self.label_to_id = {label: n for n, label in enumerate(labels)}
        self.labels = np.asarray(labels)
        self.register_tensor('points', points)
        self.register_tensor('symmetries', symmetries)
        self.__dict__['_tables'] = {}

    @property
    def n_sym_mapping(self):
        return {label: obj['n_sym'] for label, obj in self.infos.items()}

    def select(self, labels):
        ids = [self.label_to_id[l] for l in labels]
        # rows gathered with device-resident ids (cached upload, _lib.ints_to_device): indexing with the Python list would copy it to the
        # device synchronously, i.e. stop the host until every kernel queued so far has run -- once per training step
        rows = self.object_ids(labels).long() if self.points.is_cuda and len(ids) else torch.as_tensor(ids, dtype=torch.long, device=self.points.device)
        return Meshes(infos=[self.infos[l] for l in labels], labels=self.labels[ids],
                      points=torch.index_select(self.points, 0, rows), symmetries=torch.index_select(self.symmetries, 0, rows))

    # ---- device-side fast path -------------------------------------------------------------
    def object_ids(self, labels, device=None):
        """int32 row indices of `labels` in the point table."""
        from ._lib import ints_to_device
        ids = np.fromiter((self.label_to_id[l] for l in labels), dtype=np.int32, count=len(labels))
        return ints_to_device(ids, device if device is not None else self.points.device)

    def point_table(self, n_points=2000):
        """(n_obj, n_points, 3) fp32 contiguous on the points' device: points[:, deterministic ids]."""
        pts = self.points
        key = (n_points, pts.device, pts.data_ptr(), pts._version)
        tab = self._tables.get(key)
        if tab is None:
            ids = torch.as_tensor(deterministic_point_ids(pts.shape[1], n_points)).to(pts.device)
            tab = torch.index_select(pts, 1, ids).float().contiguous()
            self._tables.clear()
            self._tables[key] = tab
        return tab

    def aabb(self):
        """A BatchedMeshes of the same objects whose points are the 8 corners of each object's axis-aligned bounding box, built from
        the point table where it lies (the reference's MeshDataBase.batched(aabb=True); corner order of mesh_ops.py:15-28).  This is
        what the multi-view matching measures its distances over."""
        lo, hi = self.points.min(dim=1).values, self.points.max(dim=1).values
        pick = torch.from_numpy(_AABB_PICK).to(self.points.device)
        corners = torch.where(pick[None], hi[:, None, :], lo[:, None, :]).contiguous()
        return BatchedMeshes(self.infos, self.labels, corners, self.symmetries)

    def to(self, torch_attr):
        super().to(torch_attr)
        self._tables.clear()
        return self


def _quat_matrix(x, y, z, w):
    """rotation matrix of a unit quaternion, the product order of Eigen's toRotationMatrix (what the reference's Transform holds)"""
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, 1.0 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1.0 - (txx + tyy)]])


def make_bop_symmetries(dict_symmetries, n_symmetries_continuous=8, scale=0.001):
    """The symmetry set of a BOP object as (n,4,4) float64 (cosypose/lib3d/symmetries.py, host NumPy): the identity and the discrete
    symmetries (their translations times `scale`), and for every continuous symmetry n_symmetries_continuous rotations by 2 pi k / n
    about its axis -- a coordinate axis, offset 0, both asserted.  With continuous symmetries the set is M_c M_d for every discrete
    M_d, the continuous ones as the inner loop; without, the discrete list alone."""
    sym_discrete = dict_symmetries.get('symmetries_discrete', [])
    sym_continuous = dict_symmetries.get('symmetries_continuous', [])
    all_M_discrete, all_M_continuous = [np.eye(4)], []
    for sym_n in sym_discrete:
        M = np.array(sym_n, dtype=np.float64).reshape(4, 4)
        M[:3, -1] *= scale
        all_M_discrete.append(M)
    for sym_n in sym_continuous:
        assert np.allclose(sym_n['offset'], 0)
        axis = np.array(sym_n['axis'], dtype=np.float64)
        assert axis.shape == (3,) and axis.sum() == 1 and sorted(np.abs(axis).tolist()) == [0.0, 0.0, 1.0]       # a single 1
        for n in range(n_symmetries_continuous):
            half = axis * 2 * np.pi * n / n_symmetries_continuous / 2.0
            M = np.eye(4)
            M[:3, :3] = _quat_matrix(*np.sin(half), np.cos(half.sum()))
            all_M_continuous.append(M)
    if all_M_continuous:
        return np.array([sym_c @ sym_d for sym_d in all_M_discrete for sym_c in all_M_continuous])
    return np.array(all_M_discrete)


_UNIT_SCALE = {'mm': 0.001, 'm': 1.0}
_AABB_PICK = np.array([[0, 1, 1], [1, 1, 1], [1, 0, 1], [0, 0, 1], [0, 1, 0], [1, 1, 0], [1, 0, 0], [0, 0, 0]], dtype=bool)     # 1: max, 0: min (mesh_ops.py:15-28)


class MeshDataBase:
    """The reference's MeshDataBase over vertex arrays instead of mesh files.  obj_list: the reference's rows -- label, mesh_units
    ('mm' or 'm'), symmetries_discrete, symmetries_continuous, is_symmetric, and optionally diameter / diameter_m; verts_list: one (V,3)
    array or tensor per row, in mesh_units."""

    def __init__(self, obj_list, verts_list):
        assert len(obj_list) == len(verts_list)
        self.infos = {obj['label']: obj for obj in obj_list}
        assert len(self.infos) == len(obj_list), 'labels must be distinct'
        self.vertices = {obj['label']: v for obj, v in zip(obj_list, verts_list)}

    @staticmethod
    def from_models_info(models_info, verts_by_obj_id, mesh_units='mm'):
        """models_info: the dict of a BOP models_info.json (keys: object ids as int or str), or None; verts_by_obj_id: {obj_id: (V,3)}.
        The rows are built as the reference's BOPObjectDataset builds them (label obj_%06d, is_symmetric, diameter_m = diameter * scale),
        in the order of models_info (of verts_by_obj_id where it is None).  Objects without a `diameter` get the exact one from
        model_info, all of them in one call."""
        if mesh_units not in _UNIT_SCALE:
            raise ValueError('Unit not supported', mesh_units)
        verts_by_obj_id = {int(k): v for k, v in verts_by_obj_id.items()}
        models_info = {k: {} for k in verts_by_obj_id} if models_info is None else {int(k): v for k, v in models_info.items()}
        missing = [k for k, v in models_info.items() if 'diameter' not in v]
        computed = {}
        if missing:
            from .model_info import diameters
            computed = dict(zip(missing, diameters([verts_by_obj_id[k] for k in missing]).tolist()))
        scale = _UNIT_SCALE[mesh_units]
        objects = []
        for obj_id, bop_info in models_info.items():
            obj = dict(label=f'obj_{obj_id:06d}', category=None, mesh_units=mesh_units)
            is_symmetric = False
            for k in ('symmetries_discrete', 'symmetries_continuous'):
                obj[k] = bop_info.get(k, [])
                if len(obj[k]) > 0:
                    is_symmetric = True
            obj['is_symmetric'] = is_symmetric
            obj['diameter'] = bop_info['diameter'] if 'diameter' in bop_info else computed[obj_id]
            obj['diameter_m'] = obj['diameter'] * scale
            objects.append(obj)
        return MeshDataBase(objects, [verts_by_obj_id[k] for k in models_info])

    def batched(self, aabb=False, resample_n_points=None, n_sym=64):
        """-> BatchedMeshes with the reference's bytes: vertices scaled to metres in float64 and only then rounded to float32; shorter
        point sets padded with vertices drawn by ONE RandomState(0), in object order, consumed only by objects that need padding;
        symmetry lists padded with the identity; infos gain n_points and n_sym.  aabb=True: the 8 box corners instead (n_points = 8)."""
        if resample_n_points is not None:
            raise NotImplementedError('resample_n_points needs trimesh.sample.sample_surface, which this package does not carry')
        labels, points, symmetries = [], [], []
        new_infos = deepcopy(self.infos)
        for label, verts in self.vertices.items():
            infos = self.infos[label]
            if infos['mesh_units'] not in _UNIT_SCALE:
                raise ValueError('Unit not supported', infos['mesh_units'])
            scale = _UNIT_SCALE[infos['mesh_units']]
            points_n = np.asarray(verts.detach().cpu() if isinstance(verts, torch.Tensor) else verts).astype(np.float64)
            assert points_n.ndim == 2 and points_n.shape[1] == 3 and len(points_n) >= 1, (label, points_n.shape)
            if aabb:
                points_n = np.where(_AABB_PICK, points_n.max(0)[None], points_n.min(0)[None])
            points_n = points_n * scale
            dict_symmetries = {k: infos.get(k, []) for k in ('symmetries_discrete', 'symmetries_continuous')}
            symmetries_n = make_bop_symmetries(dict_symmetries, n_symmetries_continuous=n_sym, scale=scale)
            new_infos[label]['n_points'] = points_n.shape[0]
            new_infos[label]['n_sym'] = symmetries_n.shape[0]
            symmetries.append(symmetries_n)
            points.append(points_n)
            labels.append(label)
        rng = np.random.RandomState(0)
        n_max = max(len(p) for p in points)
        points = np.stack([p if len(p) == n_max else np.concatenate([p, p[rng.choice(np.arange(len(p)), size=n_max - len(p))]]) for p in points])
        s_max = max(len(s) for s in symmetries)
        symmetries = np.stack([np.concatenate([s, np.tile(np.eye(4), (s_max - len(s), 1, 1))]) for s in symmetries])
        return BatchedMeshes(new_infos, np.array(labels), torch.from_numpy(points), torch.from_numpy(symmetries)).float()
