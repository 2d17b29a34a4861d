"""Object models on the device: what the BOP toolkit's calc_model_info.py writes into models_info.json -- the diameter (the largest
distance between two vertices, misc.calc_pts_diameter = max(cdist(pts, pts)) in float64) and the axis-aligned box -- for a list of models
in one call.  HIP: csrc/kernels_models.hip behind cosy_model_info; DESIGN.md section 20 holds the contract, tests/models_ref.py the numpy
restatement.

The device returns the largest SQUARED distance, bit-equal to the square SciPy's cdist takes the root of, and the vertex pair that
attains it; the square root is taken here, on the host, in float64.
"""
import sys
import types

import numpy as np
import torch

from ._lib import lib, check, ptr, stream, require_device, host_to_device

TILE = 512          # vertices per tile edge of the pair kernel (MI_TILE of csrc/kernels_models.hip)
RECORD = np.dtype([('s_max', '<f8'), ('min', '<f8', (3,)), ('max', '<f8', (3,)), ('i', '<i4'), ('j', '<i4'), ('n_bad', '<i8')])      # cosy_model_info_t


def _records(verts_list):
    """the device half: -> structured array (n,) of RECORD, after the one device-to-host copy"""
    n = len(verts_list)
    if n == 0:
        return np.zeros(0, RECORD)
    verts_list = [v if isinstance(v, torch.Tensor) else np.asarray(v) for v in verts_list]
    names = {str(v.dtype).replace('torch.', '') for v in verts_list}
    if names - {'float32', 'float64'}:
        raise TypeError(f'model_info takes float32 or float64 vertices, got {sorted(names)}')
    dtype = torch.float64 if 'float64' in names else torch.float32            # a mixed list is widened, which is exact
    for k, v in enumerate(verts_list):
        if v.ndim != 2 or v.shape[1] != 3 or v.shape[0] < 1:
            raise ValueError(f'model {k}: vertices of shape {tuple(v.shape)}, expected (V, 3) with V >= 1')
    tensors = [v for v in verts_list if isinstance(v, torch.Tensor)]
    require_device(*tensors)
    dev = tensors[0].device if tensors else torch.device('cuda')
    # NumPy models are uploaded once, as one array; device models are gathered on the device
    if not tensors:
        verts = host_to_device(np.concatenate(verts_list).astype(np.float64 if dtype == torch.float64 else np.float32), dev)
    else:
        verts = torch.cat([(v.detach() if isinstance(v, torch.Tensor) else host_to_device(v, dev)).to(device=dev, dtype=dtype) for v in verts_list])
    verts = verts.contiguous()
    host_offsets = np.concatenate([[0], np.cumsum([v.shape[0] for v in verts_list])]).astype(np.int64)
    offsets = host_to_device(host_offsets, dev)
    host_p = host_offsets.ctypes.data
    ws_bytes = lib().cosy_model_info_workspace_bytes(host_p, n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    out = torch.empty(n * RECORD.itemsize, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib().cosy_model_info(ptr(verts), verts.element_size(), ptr(offsets), host_p, n, ptr(out), ptr(ws), ws_bytes, stream()))
    return out.cpu().numpy().view(RECORD)                                      # the one wait


def model_info(verts_list):
    """verts_list: list of (V_i,3) device tensors (or NumPy arrays, uploaded once), float32 or float64, in the model's own units.
    -> list of dicts with the keys of the toolkit's models_info.json -- diameter, min_x, min_y, min_z, size_x, size_y, size_z, Python
    floats in the model's units -- and diameter_ids = (i, j), i < j: the lexicographically smallest vertex pair that is a diameter
    ((0, 0) for a single vertex).  All models go through one launch set; the host waits once, for the results.  A model with a
    non-finite coordinate raises ValueError naming it."""
    rec = _records(list(verts_list))
    bad = [k for k in range(len(rec)) if rec['n_bad'][k] != 0]
    if bad:
        raise ValueError(f'model {bad[0]} has {int(rec["n_bad"][bad[0]])} non-finite coordinates' +
                         (f' (and models {bad[1:]} too)' if len(bad) > 1 else ''))
    diam = np.sqrt(rec['s_max'])
    size = rec['max'] - rec['min']                                                 # float64, as calc_3d_bbox forms it
    return [dict(diameter=float(diam[k]), min_x=float(rec['min'][k, 0]), min_y=float(rec['min'][k, 1]), min_z=float(rec['min'][k, 2]),
                 size_x=float(size[k, 0]), size_y=float(size[k, 1]), size_z=float(size[k, 2]), diameter_ids=(int(rec['i'][k]), int(rec['j'][k])))
            for k in range(len(rec))]


def diameters(verts_list):
    """-> (n,) float64: the BOP diameters, in the models' units -- what BopModels(..., diameters=...) takes"""
    return np.array([m['diameter'] for m in model_info(verts_list)], dtype=np.float64)


class _CallableModule(types.ModuleType):
    """`cosypose_amd.model_info` names this module once it is imported and the function before: calling either is the function"""

    def __call__(self, verts_list):
        return model_info(verts_list)

    __call__.__doc__ = model_info.__doc__


sys.modules[__name__].__class__ = _CallableModule
