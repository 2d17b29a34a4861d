"""numpy float64 restatements for the object models (cosypose_amd/model_info.py, csrc/kernels_models.hip, MeshDataBase): the BOP diameter
with the kernel's operation order and tie rule, the box, and a closed form of the BOP symmetry sets.  No package code."""
import numpy as np


def make_models(seed, sizes, scale=100.0, dtype=np.float32):
    """one (V,3) array per size; float32: float32-valued coordinates; float64: coordinates that no float32 holds"""
    rs = np.random.RandomState(seed)
    out = []
    for V in sizes:
        p = rs.standard_normal((V, 3)) * scale * rs.uniform(0.5, 2.0, 3)
        out.append(np.ascontiguousarray(p.astype(dtype)))
    return out


def sq_dist(a, b):
    """squared distances of a (n,3) against b (m,3) in float64: dx = x_i - x_j, then ((dx dx + dy dy) + dz dz), one rounding per operation"""
    d = np.asarray(a, np.float64)[:, None, :] - np.asarray(b, np.float64)[None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def diameter_ref(p, chunk=512):
    """-> (s_max, (i, j)): the largest squared distance over the pairs i < j of p (V,3) and the lexicographically smallest pair that
    attains it; V = 1: (0.0, (0, 0)).  Row chunks, so a model of some thousand vertices needs no V x V matrix."""
    p = np.asarray(p, np.float64)
    V = len(p)
    best, pair = -1.0, (0, 0)
    cols = np.arange(V)
    for i0 in range(0, V, chunk):
        s = sq_dist(p[i0:i0 + chunk], p)
        s[cols[None, :] <= np.arange(i0, min(V, i0 + chunk))[:, None]] = -1.0        # only j > i
        m = s.max()
        if m > best:                                                                  # rows ascend: a later chunk wins on `>` only
            i, j = np.unravel_index(np.argmax(s), s.shape)                            # argmax: the first in row-major order
            best, pair = float(m), (i0 + int(i), int(j))
    return (0.0, (0, 0)) if best < 0 else (best, pair)


def box_ref(p):
    """-> (min (3,), size (3,)) in float64, size = max - min as the toolkit's calc_3d_bbox forms it"""
    p = np.asarray(p, np.float64)
    return p.min(0), p.max(0) - p.min(0)


def info_ref(p):
    s, ids = diameter_ref(p)
    lo, size = box_ref(p)
    return dict(diameter=float(np.sqrt(s)), min_x=float(lo[0]), min_y=float(lo[1]), min_z=float(lo[2]), size_x=float(size[0]), size_y=float(size[1]),
                size_z=float(size[2]), diameter_ids=ids)


def cube(edge=2.0):
    """the 8 corners of a cube, x fastest: corner k = (k & 1, k >> 1 & 1, k >> 2) * edge.  The 4 space diagonals are (0,7), (1,6), (2,5), (3,4)"""
    k = np.arange(8)
    return np.stack([k & 1, (k >> 1) & 1, k >> 2], 1).astype(np.float32) * np.float32(edge)


def rodrigues(axis_id, theta):
    """rotation by theta about coordinate axis axis_id: R = I + sin(theta) K + (1 - cos(theta)) K^2, K the cross-product matrix of the axis"""
    a = np.zeros(3)
    a[axis_id] = 1.0
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(theta) * K + (1.0 - np.cos(theta)) * (K @ K)


def symmetries_ref(discrete, continuous_axes, n, scale):
    """the BOP symmetry set in closed form: discrete = list of 16 numbers (4x4 row-major, translation in the model's units),
    continuous_axes = list of coordinate-axis numbers.  Identity first among the discrete ones; with continuous axes every discrete
    M_d gives the run M_c M_d over all (axis, k) -- the continuous symmetry is the inner loop; without, the discrete list alone."""
    Md = [np.eye(4)]
    for d in discrete:
        M = np.array(d, np.float64).reshape(4, 4).copy()
        M[:3, 3] *= scale
        Md.append(M)
    Mc = []
    for ax in continuous_axes:
        for k in range(n):
            M = np.eye(4)
            M[:3, :3] = rodrigues(ax, 2.0 * np.pi * k / n)
            Mc.append(M)
    if not Mc:
        return np.stack(Md)
    return np.stack([c @ d for d in Md for c in Mc])


AABB_PICK = np.array([[0, 1, 1], [1, 1, 1], [1, 0, 1], [0, 0, 1], [0, 1, 0], [1, 1, 0], [1, 0, 0], [0, 0, 0]], bool)   # 1: max, 0: min


def aabb_ref(p):
    """the 8 corners of the box of p in the order of the reference's get_meshes_bounding_boxes"""
    p = np.asarray(p)
    return np.where(AABB_PICK, p.max(0)[None], p.min(0)[None])
