"""The mesh rasteriser -- kernels_raster.hip, raster_device.h and the fused render + crop + pack resolve of kernels_geom.hip --
against an independent float64 ray caster (tests/raster_ref.py), at the shapes and poses where a rasteriser goes wrong.

Until this module the rasteriser was held only to its CPU twin (oracle/cosy_oracle.c), which restates the same image-plane
arithmetic line by line: a shared mistake of thought (affine interpolation, a half-pixel slip, a transposed normal rotation, a
light in the wrong frame, a flipped texture row) passes on both sides.  Here:

  CPU suite  the twin against the ray caster on the whole case matrix -- the twin itself is now held to something, and the caps
             (exempt share, comparable pixels, the bounds) are shown to be met by the references alone;
  GPU suite  the kernel against the ray caster under the same rules, bit-equal to the twin, the fused crop path against render,
             single crops against their row in the batch, a second run against the first, non-finite poses, the C wrappers' refusals.

The rules (which pixels are comparable, the depth and colour bounds and where their constants come from) are in raster_ref.py.
"""
import ctypes

import numpy as np
import pytest
import torch

import raster_ref as R

gpu = pytest.mark.gpu
COSY_OK, COSY_EINVAL = 0, -1


# ---------------------------------------------------------------------------------------------------------------------
# CPU suite
# ---------------------------------------------------------------------------------------------------------------------
def test_ray_caster_on_an_analytic_plane():
    """The reference against a closed form: the plane z = c + a x + b y meets the ray (dx, dy, 1) t at t = c / (1 - a dx - b dy);
    the hit's barycentrics reproduce the hit point; a triangle wholly nearer than 0.01 is not seen, one across it is clipped per pixel."""
    a, b, c = 0.3, -0.2, 1.5
    xy = np.array([[-2, -2], [2, -2], [2, 2], [-2, 2]], np.float64)
    P = np.concatenate([xy, (c + a * xy[:, :1] + b * xy[:, 1:])], 1)
    faces = np.array([[0, 1, 2], [0, 2, 3]])
    K = np.array([[100., 0, 31.3], [0, 90., 20.9], [0, 0, 1]])
    depth, face, bary = R.cast(P, faces, K, 40, 64)
    ys, xs = np.mgrid[0:40, 0:64]
    for s, (ox, oy) in enumerate(R.OFFSETS):
        dx, dy = (xs + 0.5 + ox - K[0, 2]) / K[0, 0], (ys + 0.5 + oy - K[1, 2]) / K[1, 1]
        want = c / (1 - a * dx - b * dy)
        assert (face[s] >= 0).all() and np.abs(depth[s] / want - 1).max() < 1e-14
        hitp = (bary[s][..., None] * P[faces[face[s]]]).sum(-2)
        assert np.abs(hitp - np.stack([dx * want, dy * want, want], -1)).max() < 1e-13
    # near plane, per pixel: the plane z = 0.01 + y through a big triangle is met at t = 0.01 / (1 - dy): beyond 0.01 exactly where dy > 0
    P2 = np.array([[-5, -5, -4.99], [5, -5, -4.99], [0, 5, 5.01]])
    d2, f2, _ = R.cast(P2, np.array([[0, 1, 2]]), K, 40, 64, offsets=((0.0, 0.0),))
    assert np.array_equal(f2[0] >= 0, ys + 0.5 > K[1, 2]) and d2[f2 >= 0].min() > R.NEAR
    d3, f3, _ = R.cast(np.array([[-5, -5, 0.009], [5, -5, 0.009], [0, 5, 0.009]]), np.array([[0, 1, 2]]), K, 40, 64, offsets=((0.0, 0.0),))
    assert (f3 < 0).all()


@pytest.mark.parametrize('name', R.CASE_NAMES)
def test_twin_vs_ray_caster(oracle, name):
    """oracle.rasterize (the CPU twin the GPU tests require the kernel to equal) against the float64 ray caster, under the rules
    of raster_ref.compare: equal foreground decision, depth and colour within the derived bounds, exempt share <= 1 %, >= 100
    comparable pixels; the off-screen case black; the near-plane case exempt for the near rule and nothing else.

    Measured on the twin (depth ratio / colour ratio = worst deviation over bound, exempt share of the foreground):
      usual_240x320 0.29 / 0.27, 7.9e-4    b1 0.35 / 0.08, 7.7e-4          b17 0.39 / 0.33, 9.2e-4       size_45x61 0.26 / 0, 1.4e-4
      size_48x64 0.24 / 0, 2.5e-4          far 0.24 / 0.30, 1.4e-3         close_offscreen 0.24 / 0.33, 1.5e-3
      near_plane 0.20 / 0.38 (9733 of 49152 pixels near-exempt, 0 otherwise)   pp_outside 0.16 / 0.10, 1.1e-4
      f2600 0.77 / 0.21, 8.8e-5            coarse_mixed 0.40 / 0.33, 1.1e-4  interpenetrating 0.25 / 0.11, 0
      needle_fan 0.80 / 0.07, 0            padded_mixed_VF 0.24 / 0.13, 5.3e-4  mirror 0.32 / 0.12, 8.0e-4   exact_tie 0.10 / 0"""
    case = R.cases()[name]
    rgb, depth, face = case.twin(oracle)
    R.compare(case, rgb, depth, face, 'twin')


def _tie_expectations(case, rgb, depth):
    """exact_tie: every pixel centre of the closed square [4.5, 36.5]^2 is covered (no hole on the shared edges, the centre vertex or
    the outline), nothing outside is, and on a shared edge / the shared vertex the LOWER face id wins.  The colour names the face:
    ambient 1, diffuse 0, every face with its own vertices of one colour."""
    assert case.kind == 'tie'
    col = np.array([[1.0, 0.25, 0.25], [0.25, 1.0, 0.25], [0.25, 0.25, 1.0], [1.0, 1.0, 0.25]], np.float32)
    ys, xs = np.mgrid[0:40, 0:40]
    inside = (xs >= 4) & (xs <= 36) & (ys >= 4) & (ys <= 36)
    assert np.array_equal(depth[0] > 0, inside), 'hole or spill: ' + str(np.argwhere((depth[0] > 0) != inside)[:6].tolist())
    assert (depth[0][inside] == 1.0).all()
    # faces: 0 top (y < both diagonals), 1 right, 2 bottom, 3 left; membership of the closed triangles around (20, 20)
    X, Y = xs - 20, ys - 20
    member = np.stack([(Y <= X) & (Y <= -X), (X >= Y) & (X >= -Y), (Y >= X) & (Y >= -X), (X <= Y) & (X <= -Y)])
    want = np.where(inside, member.argmax(0), -1)                     # argmax of booleans: the first, i.e. the lowest, member
    got = np.full((40, 40), -1)
    img = rgb[0].transpose(1, 2, 0)
    for f in range(4):
        got[(img == col[f]).all(-1)] = f
    assert np.array_equal(got, want), np.argwhere(got != want)[:6].tolist()
    assert (member.sum(0)[inside] > 1).sum() == 2 * 33 - 1            # the ties are there: both diagonals of a 33 x 33 square


def test_exact_tie_twin(oracle):
    case = R.cases()['exact_tie']
    rgb, depth, face = case.twin(oracle)
    _tie_expectations(case, rgb, depth)
    # ... and the ray caster resolves the same ties the same way (exact arithmetic on dyadic coordinates)
    r = case.reference[0]
    assert np.array_equal(r['face'], face[0])


def test_colour_floor_is_the_float32_reference():
    """The colour floors are 3 x the deviation of the reference's OWN formula evaluated in float32 (raster_ref.FLOOR_MEASURED), not
    anything a kernel gave: re-measure, and refuse a table that has drifted from the measurement by more than a factor of two
    either way (numpy's float32 pow / sqrt may differ in the last place between builds)."""
    for name in R.CASE_NAMES:
        case = R.cases()[name]
        got, rec = R.float32_floor(case), R.FLOOR_MEASURED[name]
        print(f'  {name:18s} float32 evaluation off by {got:.2e} (recorded {rec:.2e})')
        assert rec / 2 <= got <= rec * 2 or (got == 0 and rec == 0), (name, got, rec)


def test_oracle_rasterize_does_not_normalise_the_light(oracle):
    """cosy_shade_t.light is a documented precondition (unit vector); the twin uses it as given: twice the vector, twice the
    diffuse term.  (HipBatchRenderer normalises before it fills the struct.)"""
    case = R.cases()['b1']
    m = case.meshes()
    args = (m.verts.numpy(), m.colors.numpy(), m.faces.numpy(), m.n_faces.numpy(), case.obj, case.TCO, case.K, case.H, case.W)
    l = case.light32
    a, d, _ = oracle.rasterize(*args, ambient=0.0, diffuse=0.25, light_dir=tuple(l))
    b, _, _ = oracle.rasterize(*args, ambient=0.0, diffuse=0.25, light_dir=tuple(2 * l))
    fg = d[0] > 0
    assert fg.sum() > 100 and np.abs(b[0][:, fg] - 2 * a[0][:, fg]).max() < 1e-6 and a[0][:, fg].max() > 0.05


# ---------------------------------------------------------------------------------------------------------------------
# GPU suite
# ---------------------------------------------------------------------------------------------------------------------
def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to('cuda', dtype).contiguous()


_GPU = {}


def _gpu_case(name):
    """(case, renderer, rgb, depth) of one render of the case on the device, cached for the module"""
    if name not in _GPU:
        from cosypose_amd.rasterizer import HipBatchRenderer
        case = R.cases()[name]
        renderer = HipBatchRenderer(case.meshes().cuda(), shading=case.shading)
        # every side gets the same unit float32 light
        assert np.array_equal(np.array(list(renderer.shade.light), np.float32), case.light32)
        rgb, depth = renderer.render(case.infos(), dev(case.TCO), dev(case.K), resolution=(case.H, case.W), render_depth=True)
        torch.cuda.synchronize()
        _GPU[name] = (case, renderer, rgb, depth)
    return _GPU[name]


def _equal_to_twin(case, rgb, depth, t_rgb, t_depth):
    """depth bit for bit; rgb bit for bit, except where powf is involved (specular > 0): the tolerance that
    test_rasteriser_opengl_like_shading_vs_cpu_twin grants -- one 8-bit step at most, on fewer than 1e-3 of the values"""
    assert np.array_equal(depth.view(np.uint32), t_depth.view(np.uint32)), (case.name, int((depth != t_depth).sum()))
    if case.shading['specular'] > 0:
        diff = np.abs(rgb - t_rgb)
        assert diff.max() <= 1 / 255 + 1e-6 and (diff > 1e-6).mean() < 1e-3, (case.name, float(diff.max()), float((diff > 1e-6).mean()))
    else:
        assert np.array_equal(rgb.view(np.uint32), t_rgb.view(np.uint32)), (case.name, float(np.abs(rgb - t_rgb).max()))


@gpu
@pytest.mark.parametrize('name', R.CASE_NAMES)
def test_kernel_vs_ray_caster_and_twin(oracle, name):
    """HipBatchRenderer.render(..., render_depth=True) against the float64 ray caster under the rules the twin is held to on the CPU
    (raster_ref.compare), and bit-equal to the twin (the winning face ids are the twin's: equal depth bits in every pixel)."""
    case, renderer, rgb, depth = _gpu_case(name)
    rgb, depth = rgb.cpu().numpy(), depth.cpu().numpy()
    assert rgb.shape == (case.B, 3, case.H, case.W) and depth.shape == (case.B, case.H, case.W)
    t_rgb, t_depth, t_face = case.twin(oracle)
    R.compare(case, t_rgb, t_depth, t_face, 'twin')
    R.compare(case, rgb, depth, t_face, 'kernel')
    _equal_to_twin(case, rgb, depth, t_rgb, t_depth)
    if case.kind == 'tie':
        _tie_expectations(case, rgb, depth)


@gpu
@pytest.mark.parametrize('name', R.CASE_NAMES)
def test_single_crops_and_rerun_equal_the_batch(name):
    """Each crop rendered alone (B = 1) equals its row in the batch bit for bit, and a second run of the batch equals the first."""
    case, renderer, rgb, depth = _gpu_case(name)
    rgb2, depth2 = renderer.render(case.infos(), dev(case.TCO), dev(case.K), resolution=(case.H, case.W), render_depth=True)
    assert torch.equal(rgb2.view(torch.int32), rgb.view(torch.int32)) and torch.equal(depth2.view(torch.int32), depth.view(torch.int32))
    infos = case.infos()
    for b in range(case.B):
        r1, d1 = renderer.render(infos[b:b + 1], dev(case.TCO[b:b + 1]), dev(case.K[b:b + 1]), resolution=(case.H, case.W), render_depth=True)
        assert torch.equal(r1[0].view(torch.int32), rgb[b].view(torch.int32)), (name, b)
        assert torch.equal(d1[0].view(torch.int32), depth[b].view(torch.int32)), (name, b)


def _crop_inputs(B, seed=2, n_im=3, h=60, w=80):
    from cosypose_amd._lib import lib, check, ptr, stream
    rs = np.random.RandomState(seed)
    frames = torch.rand(n_im, 3, h, w, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1))
    frames4 = torch.empty(n_im, h, w, 4, device='cuda')
    check(lib().cosy_frames_to_nhwc4(ptr(frames), ptr(frames4), n_im, h, w, stream()))
    im_ids = torch.tensor(rs.randint(0, n_im, B), dtype=torch.int32, device='cuda')
    x1 = rs.uniform(0, 30, B); y1 = rs.uniform(0, 20, B)
    boxes = dev(np.stack([x1, y1, x1 + rs.uniform(20, 45, B), y1 + rs.uniform(15, 35, B)], 1).astype(np.float32))
    return frames4, im_ids, boxes


@gpu
@pytest.mark.parametrize('dtype', ['fp32', 'fp16', 'bf16'])
@pytest.mark.parametrize('name', R.CASE_NAMES)
def test_render_crop_pack_equals_render(name, dtype):
    """cosy_render_crop_pack_to on every case: channels 3:6 of the NHWC8 buffer are render's rgb (in NHWC) bit for bit in fp32 and
    rgb.to(dtype) bit for bit in fp16 / bf16; channels 6:8 are zero (the buffer starts as ones: they are written, not assumed);
    channels 0:3 are what cosy_crop_pack_to writes for the same frames and boxes."""
    from cosypose_amd._lib import lib, check, ptr, stream, COSY_F32, COSY_BF16, COSY_F16
    case, renderer, rgb, depth = _gpu_case(name)
    code, tdt, idt = {'fp32': (COSY_F32, torch.float32, torch.int32), 'fp16': (COSY_F16, torch.float16, torch.int16),
                      'bf16': (COSY_BF16, torch.bfloat16, torch.int16)}[dtype]
    frames4, im_ids, boxes = _crop_inputs(case.B)
    B, H, W = case.B, case.H, case.W
    got = torch.ones(B, H, W, 8, device='cuda', dtype=tdt)
    renderer.render_crop_pack(case.infos(), dev(case.TCO), dev(case.K), frames4, im_ids, boxes, (H, W), x8=got, dtype=code)
    want = torch.ones(B, H, W, 8, device='cuda', dtype=tdt)
    check(lib().cosy_crop_pack_to(ptr(want), code, ptr(frames4), ptr(im_ids), ptr(boxes), ptr(rgb.contiguous()), B, frames4.shape[0], frames4.shape[1],
                                  frames4.shape[2], H, W, stream()))
    torch.cuda.synchronize()
    nhwc = rgb.permute(0, 2, 3, 1).contiguous().to(tdt)
    assert torch.equal(got[..., 3:6].contiguous().view(idt), nhwc.view(idt)), (name, dtype)
    assert bool((got[..., 6:8] == 0).all()), (name, dtype)
    assert torch.equal(got[..., 0:3].contiguous().view(idt), want[..., 0:3].contiguous().view(idt)), (name, dtype)
    if case.kind == 'object':
        assert (got[..., 3:6].float().abs().sum(dim=(1, 2, 3)) > 0).all()


@gpu
@pytest.mark.parametrize('what', ['nan_in_TCO', 'nan_in_K_only', 'inf_in_TCO_row4'])
def test_non_finite_crop_is_black_and_alone(what):
    """A crop with a NaN in TCO, a NaN in K alone, or an Inf in TCO's fourth row is black with zero depth (bullet_batch_renderer.py:25-36
    skips such poses), in render and in the fused crop path; its neighbours in the batch are unchanged bit for bit."""
    from cosypose_amd._lib import COSY_F32
    case, renderer, rgb, depth = _gpu_case('padded_mixed_VF')
    TCO, K = case.TCO.copy(), case.K.copy()
    bad = 2
    if what == 'nan_in_TCO':
        TCO[bad, 1, 2] = np.nan
    elif what == 'nan_in_K_only':
        K[bad, 0, 2] = np.nan
    else:
        TCO[bad, 3, 1] = np.inf
    r, d = renderer.render(case.infos(), dev(TCO), dev(K), resolution=(case.H, case.W), render_depth=True)
    assert bool((rgb[bad] != 0).any())                                       # the clean crop does show its object
    assert bool((r[bad] == 0).all()) and bool((d[bad] == 0).all())
    keep = [b for b in range(case.B) if b != bad]
    assert torch.equal(r[keep].view(torch.int32), rgb[keep].view(torch.int32)) and torch.equal(d[keep].view(torch.int32), depth[keep].view(torch.int32))
    frames4, im_ids, boxes = _crop_inputs(case.B)
    x8 = torch.ones(case.B, case.H, case.W, 8, device='cuda')
    renderer.render_crop_pack(case.infos(), dev(TCO), dev(K), frames4, im_ids, boxes, (case.H, case.W), x8=x8, dtype=COSY_F32)
    torch.cuda.synchronize()
    assert bool((x8[bad, ..., 3:8] == 0).all())
    assert torch.equal(x8[keep][..., 3:6].contiguous().view(torch.int32), rgb[keep].permute(0, 2, 3, 1).contiguous().view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------------
# wrapper contract (as test_wrapper_contract of test_geom_dist_kernels.py)
# ---------------------------------------------------------------------------------------------------------------------
_MESH_PTRS = ('verts', 'colors', 'faces', 'n_faces')


def _render_call(entry, lib, pin, pout, stream, mesh=None, shade=None, **over):
    """one call of `entry` with good small arguments, `over` replacing some; mesh / shade: dicts of struct fields to replace, or
    the string 'null' for a null struct pointer"""
    from cosypose_amd._lib import MeshSet, Shade, COSY_F32
    mf = dict(verts=pin, colors=pin, normals=pin, uvs=None, tex=None, faces=pin, n_faces=pin, V=4, F=2, TH=0, TW=0)
    sf = dict(ambient=0.5, diffuse=0.5, specular=0.0, shininess=1.0, light=(ctypes.c_float * 3)(0, 0, -1), light_frame=0, smooth=0, quantize=0)
    m = None if mesh == 'null' else MeshSet(**dict(mf, **(mesh or {})))
    s = None if shade == 'null' else Shade(**dict(sf, **(shade or {})))
    mp, sp = (ctypes.byref(m) if m is not None else None), (ctypes.byref(s) if s is not None else None)
    if entry == 'render_meshes_ex':
        a = dict(obj_id=pin, TCO=pin, K=pin, B=2, H=8, W=8, rgb=pout, depth=pout + 4096, scratch=pout + 8192)
        a.update(over)
        return lib.cosy_render_meshes_ex(mp, sp, a['obj_id'], a['TCO'], a['K'], a['B'], a['H'], a['W'], a['rgb'], a['depth'], a['scratch'], stream())
    if entry == 'render_meshes':
        a = dict(verts=pin, colors=pin, faces=pin, n_faces=pin, obj_id=pin, TCO=pin, K=pin, B=2, V=4, F=2, H=8, W=8, rgb=pout, depth=pout + 4096,
                 scratch=pout + 8192)
        a.update(over)
        return lib.cosy_render_meshes(a['verts'], a['colors'], a['faces'], a['n_faces'], a['obj_id'], a['TCO'], a['K'], a['B'], a['V'], a['F'], a['H'],
                                      a['W'], 0.5, 0.5, 0.0, 0.0, -1.0, a['rgb'], a['depth'], a['scratch'], stream())
    a = dict(x_nhwc8=pout, dtype=COSY_F32, obj_id=pin, TCO=pin, K_crop=pin, frames_nhwc4=pin, im_id=None, boxes_crop=pin, B=2, N=2, h=4, w=4, H=8, W=8,
             scratch=pout + 8192)
    a.update(over)
    return lib.cosy_render_crop_pack_to(a['x_nhwc8'], a['dtype'], mp, sp, a['obj_id'], a['TCO'], a['K_crop'], a['frames_nhwc4'], a['im_id'],
                                        a['boxes_crop'], a['B'], a['N'], a['h'], a['w'], a['H'], a['W'], a['scratch'], stream())


@gpu
@pytest.mark.parametrize('entry', ['render_meshes', 'render_meshes_ex', 'render_crop_pack_to'])
def test_render_wrapper_contract(entry):
    """cosy_render_meshes, cosy_render_meshes_ex and cosy_render_crop_pack_to refuse, with COSY_EINVAL and a cosy_last_error() that
    names the argument, before anything is launched: B < 0; B = 65536 (the batch is the grid's y dimension, 65535 the hardware's
    limit -- the launch used to fail inside the runtime); H, W, V, F (and h, w of the frames) <= 0; each required pointer null,
    also inside the mesh struct; smooth shading without normals; a texture without uvs or without its size.  B = 0 is COSY_OK
    with every data pointer null; depth = NULL is COSY_OK; the good call is COSY_OK.  No refused call writes the outputs."""
    from cosypose_amd._lib import lib as _lib, stream
    lib = _lib()
    inb, outb = torch.zeros(1 << 15, device='cuda'), torch.zeros(1 << 15, device='cuda')       # zeroed: every id 0, every pose singular
    pin, pout = inb.data_ptr(), outb.data_ptr()
    ex = entry != 'render_meshes'                                                               # takes the structs

    def call(**kw):
        return _render_call(entry, lib, pin, pout, stream, **kw)

    def refused(what, needle, **kw):
        rc = call(**kw)
        msg = lib.cosy_last_error().decode()
        print(f'  {entry} {what}: rc {rc}, "{msg}"')
        assert rc == COSY_EINVAL, (entry, what, rc)
        assert needle in msg, (entry, what, msg)

    assert call() == COSY_OK, lib.cosy_last_error()
    torch.cuda.synchronize()
    assert bool((outb[:2048] == 0).all())           # empty meshes: black and zero depth (the scratch lies 8192 bytes on)
    outb.fill_(7.0)
    torch.cuda.synchronize()
    refused('B = -1', 'B=-1', B=-1)
    refused('B = 65536', 'B=65536', B=65536)
    sizes = ['H', 'W'] + (['h', 'w'] if entry == 'render_crop_pack_to' else [])
    for n in sizes:
        for v in (0, -1):
            refused(f'{n} = {v}', f'{n}={v}', **{n: v})
    for n in ('V', 'F'):
        for v in (0, -1):
            refused(f'{n} = {v}', f'{n}={v}', **({'mesh': {n: v}} if ex else {n: v}))
    for n in _MESH_PTRS:
        refused(f'{n} = null', f'null {n}', **({'mesh': {n: None}} if ex else {n: None}))
    pointers = {'render_meshes': ('obj_id', 'TCO', 'K', 'rgb', 'scratch'), 'render_meshes_ex': ('obj_id', 'TCO', 'K', 'rgb', 'scratch'),
                'render_crop_pack_to': ('x_nhwc8', 'obj_id', 'TCO', 'K_crop', 'frames_nhwc4', 'boxes_crop', 'scratch')}[entry]
    for n in pointers:
        refused(f'{n} = null', f'null {n}', **{n: None})
    if ex:
        refused('mesh = null', 'null mesh', mesh='null')
        refused('shade = null', 'null shade', shade='null')
        refused('smooth without normals', 'null normals', mesh=dict(normals=None), shade=dict(smooth=1))
        refused('texture without uvs', 'uvs null', mesh=dict(tex=pin, uvs=None, TH=4, TW=4))
        refused('texture without size', 'TH=0', mesh=dict(tex=pin, uvs=pin, TH=0, TW=4))
        refused('texture without size', 'TW=0', mesh=dict(tex=pin, uvs=pin, TH=4, TW=0))
    if entry == 'render_crop_pack_to':
        refused('dtype = 7', 'dtype 7', dtype=7)
    torch.cuda.synchronize()
    assert bool((outb == 7.0).all()) and bool((inb == 0).all())                               # no refused call wrote anything
    # an empty batch is fine with every data pointer null
    null = {n: None for n in pointers}
    assert call(B=0, **null) == COSY_OK, lib.cosy_last_error()
    if entry != 'render_crop_pack_to':
        assert call(depth=None) == COSY_OK, lib.cosy_last_error()                                # depth is optional
    torch.cuda.synchronize()
    assert bool((outb[1024:2048] == 7.0).all())                                                  # ... and then not written (4096 bytes on)
