"""ctypes binding of libcosyhip.so (the C ABI declared in include/cosyhip.h).

The header is the declaration: every entry point's argtypes / restype are read from its prototype (parse_header below), so a new
entry point needs the header and its C definition and nothing here.  The header's constants and the structs that cross the
boundary are restated below, once each; tests/test_c_abi.py holds them against the header with the C compiler.

There is no fallback: if the HIP library is missing or a call fails, this raises.
"""
import ctypes
import os
import re

import torch

from .build import LIB, HEADER


class CosyHipError(RuntimeError):
    pass


_lib = None

_c = ctypes
_P, _I, _F, _D = _c.c_void_p, _c.c_int, _c.c_float, _c.c_double

_SCALARS = {'int': _I, 'unsigned': _c.c_uint, 'unsigned int': _c.c_uint, 'float': _F, 'double': _D, 'long': _c.c_long,
            'unsigned long': _c.c_ulong, 'long long': _c.c_longlong, 'unsigned long long': _c.c_ulonglong, 'size_t': _c.c_size_t,
            'cosy_stream_t': _P}
_PROTOTYPE = re.compile(r'([\w\s*]+?)\b(cosy_\w+)\s*\(([^()]*)\)\s*;')


def parse_header(text):
    """C prototypes `<ret> cosy_name(<params>);` -> {name: (argtypes, restype)} in the order they are declared.  Anything with `*` or
    `[]` is a c_void_p (device pointers, handles, struct pointers, pointers to pointers); a scalar maps by _SCALARS; a type that is in
    neither group raises and names the declaration."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
    text = re.sub(r'^[ \t]*#.*$', '', text, flags=re.M)

    def ctype(decl, name, what):
        words = [w for w in decl.replace('*', ' * ').split() if w != 'const']
        if '*' in words or '[' in decl:
            if what == 'return type':       # the one pointer the ABI returns is cosy_last_error()'s message
                if words != ['char', '*']:
                    raise CosyHipError(f'cosyhip.h: {name}: unsupported {what} `{decl.strip()}`')
                return _c.c_char_p
            return _P
        for n in (len(words), len(words) - 1):          # without and with the parameter's name
            if ' '.join(words[:n]) in _SCALARS:
                return _SCALARS[' '.join(words[:n])]
        raise CosyHipError(f'cosyhip.h: {name}: unsupported {what} `{decl.strip()}`')

    out = {}
    for ret, name, params in _PROTOTYPE.findall(text):
        params = [] if params.strip() in ('', 'void') else params.split(',')
        out[name] = ([ctype(p, name, 'parameter') for p in params], ctype(ret, name, 'return type'))
    return out


with open(HEADER) as _f:
    _SIGNATURES = parse_header(_f.read())
EXPORTS = tuple(_SIGNATURES)

# ---- the header's constants, under its names without the COSY_ prefix (COSY_F32 ... and COSY_MASK_* keep it: they are imported under it) ----
COSY_F32, COSY_BF16, COSY_F16 = 0, 1, 2
DTYPES = {torch.float32: COSY_F32, torch.bfloat16: COSY_BF16, torch.float16: COSY_F16}      # torch dtype -> storage type of a kernel
COSY_MASK_U8, COSY_MASK_I32 = 0, 1
AUG_GATE, AUG_SHARPNESS, AUG_CONTRAST, AUG_BRIGHTNESS, AUG_COLOR, AUG_GRAY = 1, 2, 4, 8, 16, 32
RESIZE_BILINEAR, RESIZE_BICUBIC = 2, 3
RPN_MAX_LEVELS, RPN_MAX_ANCHORS = 8, 16
DT_MAX_GT, DT_MAX_BATCH, DT_MAX_CLASSES, DT_MAX_M = 1024, 4096, 4096, 128
DETIN_ONE_TAP = 1
HEAD_STORE_ROWS, HEAD_STORE_NCHW, HEAD_STORE_DECONV_ROWS, HEAD_STORE_DECONV_NCHW = 0, 1, 2, 3
TRUNK_ADD_NONE, TRUNK_ADD_SAME, TRUNK_ADD_EVEN, TRUNK_ADD_NEAREST_T = 0, 1, 2, 3


class MeshSet(ctypes.Structure):       # cosy_mesh_t
    _fields_ = [('verts', _P), ('colors', _P), ('normals', _P), ('uvs', _P), ('tex', _P), ('faces', _P), ('n_faces', _P),
                ('V', _I), ('F', _I), ('TH', _I), ('TW', _I)]


class Shade(ctypes.Structure):         # cosy_shade_t
    _fields_ = [('ambient', _F), ('diffuse', _F), ('specular', _F), ('shininess', _F), ('light', _F * 3),
                ('light_frame', _I), ('smooth', _I), ('quantize', _I)]


class BaCtrl(ctypes.Structure):        # cosy_ba_ctrl_t
    _fields_ = [('loss', _D), ('next_loss', _D), ('lambd', _D), ('done', _I), ('prev_update', _I), ('finished', _I), ('n_hist', _I)]


class BaBatch(ctypes.Structure):       # cosy_ba_batch_t
    _fields_ = [(k, _I) for k in ('G', 'n_cand', 'n_obj', 'n_views', 'n_mesh', 'P', 'S', 'max_blocks', 'n_hist_rows', 'optimize_cameras')] + [
        ('a_total', _c.c_longlong)] + [(k, _D) for k in ('residuals_threshold', 'L_down', 'L_up', 'eps')] + [
        (k, _P) for k in ('table', 'cand_TCO', 'K', 'pts_table', 'sym_table', 'n_sym', 'TWO_9d', 'TCW_9d', 'TWO_9d_updated', 'TCW_9d_updated',
                          'ctrl', 'hist_iteration', 'hist_lambda', 'hist_loss', 'hist_TWO_9d', 'hist_TCW_9d', 'workspace')]


class RpnLevels(ctypes.Structure):     # cosy_rpn_levels_t
    _fields_ = [('objectness', _P * RPN_MAX_LEVELS), ('deltas', _P * RPN_MAX_LEVELS), ('H', _I * RPN_MAX_LEVELS), ('W', _I * RPN_MAX_LEVELS),
                ('stride_h', _F * RPN_MAX_LEVELS), ('stride_w', _F * RPN_MAX_LEVELS), ('base', _F * 4 * RPN_MAX_ANCHORS * RPN_MAX_LEVELS)]


class MsroiLevels(ctypes.Structure):   # cosy_msroi_levels_t
    _fields_ = [('feat', _P * RPN_MAX_LEVELS), ('H', _I * RPN_MAX_LEVELS), ('W', _I * RPN_MAX_LEVELS), ('scale', _F * RPN_MAX_LEVELS)]


class HeadLayer(ctypes.Structure):     # cosy_head_layer_t
    _fields_ = [('x', _P), ('w', _P), ('bias', _P), ('out', _P), ('out1', _P)] + [
        (k, _I) for k in ('dtype', 'ksize', 'c_in', 'c_out', 'relu', 'store', 'n_split', 'n_levels')] + [
        ('row_start', _I * (RPN_MAX_LEVELS + 1)), ('H', _I * RPN_MAX_LEVELS), ('W', _I * RPN_MAX_LEVELS)]


class ProfRec(ctypes.Structure):       # cosy_prof_rec_t
    _fields_ = [('name', _c.c_char * 64), ('layer', _I), ('n', _I), ('ms_avg', _F), ('ms_min', _F),
                ('bytes', _c.c_double), ('flops', _c.c_double), ('cbytes', _c.c_double)]


def profile_read(handle):
    """-> list of dicts, one per launch slot of the backbone schedule (see cosy_prof_rec_t)."""
    recs = (ProfRec * 1100)()
    n = _I(0)
    check(lib().cosy_effnet_b3_profile_read(handle, recs, 1100, ctypes.byref(n)))
    return [dict(name=r.name.decode(), layer=r.layer, n=r.n, ms_avg=r.ms_avg, ms_min=r.ms_min, bytes=r.bytes, flops=r.flops, cbytes=r.cbytes)
            for r in recs[:n.value]]


def lib():
    """Load the shared library (once).  Raises if it has not been built."""
    global _lib
    if _lib is None:
        path = LIB
        if os.environ.get('COSY_TUNE_LIB'):       # experiments only: the -DCOSY_TUNE build that reads COSY_* knobs (or, for A/B
            from .build import TUNE_LIB as path   # runs inside one gpurun call, another build of it given by its path)
            if os.environ['COSY_TUNE_LIB'].endswith('.so'):
                path = os.environ['COSY_TUNE_LIB']
        if not os.path.exists(path):
            raise CosyHipError(f'{path} not found: build it with `python -m cosypose_amd.build` '
                               '(or __graft_entry__.build()); cosypose_amd has no CPU / eager fallback')
        if path == LIB:
            # the wave kernels keep values in registers hipcc is not told about; only a library whose ISA was checked at build time
            # (cosypose_amd/build.py stamps the verdict with the library's hash) is loaded -- never a lazily rebuilt, unchecked one
            from .build import stamp_matches, ISA_STAMP
            if not stamp_matches(path):
                raise CosyHipError(f'{path} has no matching clean wave-kernel ISA stamp ({ISA_STAMP}): it was not produced by '
                                   '`python -m cosypose_amd.build` / __graft_entry__.build() as it stands -- rebuild')
        l = ctypes.CDLL(path)
        for name, (args, res) in _SIGNATURES.items():
            fn = getattr(l, name)
            fn.argtypes = args
            fn.restype = res
        _lib = l
    return _lib


def rows_entry(name, dtype):
    """the detector backward's entry point `name` for rows of dtype: the float32 symbol, or its `16` twin for bfloat16 rows"""
    if dtype not in (torch.float32, torch.bfloat16):
        raise CosyHipError(f'{name}: the rows of the backward are float32 or bfloat16, got {dtype}')
    return getattr(lib(), name if dtype == torch.float32 else name + '16')


def check(rc):
    if rc != 0:
        raise CosyHipError(f'libcosyhip error {rc}: {lib().cosy_last_error().decode()}')


def ptr(t):
    """Device pointer of a contiguous torch tensor (or None)."""
    return None if t is None else t.data_ptr()


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def require_device(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise CosyHipError('cosypose_amd runs on a ROCm device only (got a CPU tensor); there is no CPU fallback')


def out_or_new(out, what, shape, dtype, device, empty=None):
    """`out` (`what` in a refusal) if it is a contiguous `shape` `dtype` tensor on `device`; for None a new one from `empty` (torch.empty)"""
    import torch
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device) if empty is None else empty(shape, dtype, device)
    require_device(out)
    if out.dtype != dtype or tuple(out.shape) != tuple(shape) or not out.is_contiguous() or out.device != device:
        raise ValueError(f'{what} must be a contiguous {str(dtype)[6:]} tensor of shape {tuple(shape)} on {device}')
    return out


import collections as _collections

_id_cache = _collections.OrderedDict()       # (device index, shape, bytes) -> int32 device tensor
_ID_CACHE_ENTRIES, _ID_CACHE_MAX_BYTES = 64, 64 << 10


def host_to_device(values, device, dtype=None):
    """numpy array / CPU tensor -> device tensor through page-locked memory and a non-blocking copy: the host does not wait for the
    kernels already queued on the stream (torch's .to(device) of pageable memory does)."""
    import numpy as np
    import torch
    host = values if isinstance(values, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(values))
    if dtype is not None:
        host = host.to(dtype)
    if torch.device(device).type == 'cpu' or host.numel() == 0 or host.device.type != 'cpu':
        return host.to(device)
    return host.pin_memory().to(device, non_blocking=True)


def ints_to_device(values, device):
    """int32 device tensor from host ids (list / numpy / CPU tensor) without draining the stream: the ids go through
    pinned memory and a non-blocking copy, so the host keeps running ahead of the GPU (a pageable H2D copy would wait
    for every kernel already queued on the stream).  Device tensors are only cast."""
    import numpy as np
    import torch
    if values is None:
        return None
    if isinstance(values, torch.Tensor) and values.device.type != 'cpu':
        return values.to(device=device, dtype=torch.int32).contiguous()
    arr = np.ascontiguousarray(np.asarray(values.cpu() if isinstance(values, torch.Tensor) else values), dtype=np.int32)
    host = torch.as_tensor(arr)
    if torch.device(device).type == 'cpu' or host.numel() == 0:
        return host.to(device)
    # Small id arrays (labels -> object rows, frame ids) repeat from call to call -- the refiner's four iterations and every step of a
    # served workload hand over the same ones: keyed by CONTENT, the device copy is reused and no copy packet enters the compute stream
    # (each one stalls it for a DMA round trip).  Read-only by contract: callers pass these to kernels as inputs.
    if arr.nbytes <= _ID_CACHE_MAX_BYTES:
        key = (torch.device(device).index, arr.shape, arr.tobytes())
        hit = _id_cache.get(key)
        if hit is not None:
            _id_cache.move_to_end(key)
            dev_t, ready, home = hit
            # the upload was enqueued on the stream that first asked for this content: another stream (a concurrent chunk with the same
            # ids) must not read it before it has landed, and the caching allocator -- which would hand the block back to the HOME stream's
            # pool the moment the entry is evicted -- must know that this stream reads it too
            cur = torch.cuda.current_stream(device)
            if not ready.query():
                cur.wait_event(ready)
            if cur.cuda_stream != home:
                dev_t.record_stream(cur)
            return dev_t
        dev_t = host.pin_memory().to(device, non_blocking=True)
        ready = torch.cuda.Event()
        cur = torch.cuda.current_stream(device)
        ready.record(cur)
        _id_cache[key] = (dev_t, ready, cur.cuda_stream)
        while len(_id_cache) > _ID_CACHE_ENTRIES:
            _id_cache.popitem(last=False)
        return dev_t
    return host.pin_memory().to(device, non_blocking=True)
