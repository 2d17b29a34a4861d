"""The detector's optimiser: torch.optim.SGD(lr, momentum, weight_decay) as the reference builds it
(cosypose/training/train_detector.py:214: dampening 0, no Nesterov, torch 1.3's first-step rule) on ONE flat float32 buffer.

A step is the gradient norm the reference logs (cosy_grad_norm_clip with max_norm 0: clip_grad_norm_(max_norm=inf) never scales), the update
(cosy_sgd_step, csrc/kernels_detopt.hip) and ONE launch that repacks the packings of every trainable layer from the moved parameters
(cosy_pack_table_run over a table built once): the layers' own per-layer packs of the next forward do not run.

The bookkeeping -- re-homing the parameters and their .grad as views of flat buffers, collecting gradients that were detached from them,
zero_grad -- is plain torch and works on any device; step() needs the ROCm device, there is no CPU fallback.
"""
import ctypes

import torch

from . import _lib
from .detector_heads import PackedOnDevice

ALIGN = 4          # float32 elements: every view starts on a 16-byte boundary, as the kernels' 16-byte accesses and the packs' checks want


def _params_of(params_or_detector):
    named = getattr(params_or_detector, 'named_parameters', None)
    params = [p for _, p in named()] if named is not None else list(params_or_detector)
    if not params:
        raise ValueError('FlatSGD: no parameters')
    for i, p in enumerate(params):
        if not isinstance(p, torch.Tensor) or p.dtype != torch.float32:
            raise ValueError(f'FlatSGD: parameter {i} must be a float32 tensor, got {getattr(p, "dtype", type(p).__name__)}')
        if p.device != params[0].device:
            raise ValueError(f'FlatSGD: parameter {i} lives on {p.device}, parameter 0 on {params[0].device}: one flat buffer, one device')
    if len({id(p) for p in params}) != len(params):
        raise ValueError('FlatSGD: a parameter is listed twice')
    return params


def table_row(layer):
    """a PackedOnDevice layer -> the 13 words of its row: its pack_args(), its three packings and the type of its rows"""
    w0, b0, w1, b1, scale, ksize, c_in, n0, n1 = layer.pack_args()
    want = layer.packed_sizes(ksize, c_in, n0, n1, layer.dtype)          # the buffers the launch writes must hold what it writes
    have = (layer.w.numel(), layer.bias.numel(), layer.w_t.numel())
    if have != want or layer.w.dtype != layer.dtype or layer.w_t.dtype != layer.dtype or layer.bias.dtype != torch.float32:
        raise ValueError(f'FlatSGD: a layer\'s packings hold {have} elements of {layer.w.dtype}, its pack writes {want} of {layer.dtype}')
    ptr = lambda t: 0 if t is None else t.data_ptr()
    return [ptr(w0), ptr(b0), ptr(w1), ptr(b1), ptr(scale), ptr(layer.w), ptr(layer.bias), ptr(layer.w_t), ksize, c_in, n0, n1, _lib.DTYPES[layer.dtype]]


class PackTable:
    """The packings of `layers` (PackedOnDevice) rewritten by one launch: rows validated by the library and uploaded once, here."""

    def __init__(self, layers):
        self.layers = list(layers)
        if not self.layers:
            raise ValueError('PackTable: no layers')
        dev = self.layers[0].device
        rows = [w for layer in self.layers for w in table_row(layer)]
        L = _lib.lib()
        n = len(self.layers)
        self.table = torch.empty(L.cosy_pack_table_bytes(n), dtype=torch.uint8, device=dev)
        wgs = ctypes.c_longlong(0)
        with torch.cuda.device(dev):
            _lib.check(L.cosy_pack_table_build((ctypes.c_longlong * len(rows))(*rows), n, _lib.ptr(self.table), self.table.numel(), ctypes.byref(wgs), _lib.stream()))
        self.n_workgroups = wgs.value
        self.home = [tuple(p.data_ptr() for p in layer.parameters()) for layer in self.layers]       # where the table reads the parameters

    def run(self):
        for layer, home in zip(self.layers, self.home):
            if tuple(p.data_ptr() for p in layer.parameters()) != home:
                raise RuntimeError('PackTable: a parameter has moved to other memory since the table was built (.data was replaced): build the optimiser again')
        with torch.cuda.device(self.table.device):
            _lib.check(_lib.lib().cosy_pack_table_run(_lib.ptr(self.table), len(self.layers), self.n_workgroups, _lib.stream()))


class FlatSGD:
    """FlatSGD(params_or_detector, lr, momentum=0.9, weight_decay=1e-4, layers=None).

    Construction re-homes the parameters as views of one flat float32 buffer (`flat`) and their .grad as views of `grad`, in
    named_parameters() order; the Parameter objects stay the same objects, their values the same bits; every view starts 16-byte aligned and
    the padding elements hold +0.0 and stay so (their gradient is zero, so is their update).  param_groups = [{'lr': ...}] is read by step():
    training.LRSchedule.apply and user code set the rate there as on a torch optimiser.
    layers: the PackedOnDevice layers whose packings step() keeps current (Detector.optimizer() gives the detector's trainable ones)."""

    def __init__(self, params_or_detector, lr, momentum=0.9, weight_decay=1e-4, layers=None):
        if lr < 0 or momentum < 0 or weight_decay < 0:
            raise ValueError(f'FlatSGD: lr={lr}, momentum={momentum} and weight_decay={weight_decay} must be >= 0')
        params = self.params = _params_of(params_or_detector)
        dev = params[0].device
        self.offsets, off = [], 0
        for p in params:
            self.offsets.append(off)
            off += -(-p.numel() // ALIGN) * ALIGN
        n = off
        self.flat = torch.zeros(n, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(n, dtype=torch.float32, device=dev)
        if self.flat.data_ptr() % 16 or self.grad.data_ptr() % 16:
            raise RuntimeError('FlatSGD: the allocator returned a buffer that is not 16-byte aligned')
        with torch.no_grad():
            for p, o in zip(params, self.offsets):
                view = self.flat[o:o + p.numel()].view(p.shape)
                view.copy_(p.data)
                old = p.grad
                p.data = view
                p.grad = None
                p.grad = self.grad[o:o + p.numel()].view(p.shape)
                if old is not None:
                    p.grad.copy_(old)
        self.momentum, self.weight_decay = float(momentum), float(weight_decay)
        self.param_groups = [{'lr': float(lr), 'momentum': self.momentum, 'weight_decay': self.weight_decay, 'params': params}]
        self.momentum_buffer = torch.zeros(n, dtype=torch.float32, device=dev) if self.momentum != 0 else None
        self.norm_coef = torch.ones(2, dtype=torch.float32, device=dev)
        self.step_count = 0
        self.layers = [] if layers is None else list(layers)
        mine = {id(p) for p in params}
        for layer in self.layers:
            if not isinstance(layer, PackedOnDevice):
                raise ValueError(f'FlatSGD: layers holds a {type(layer).__name__}; only trainable layers (PackedOnDevice) pack on the device')
            if any(id(p) not in mine for p in layer.parameters()):
                raise ValueError('FlatSGD: a layer\'s parameter is not among the optimiser\'s parameters: its packing would follow a buffer the step never writes')
        self.table = PackTable(self.layers) if self.layers else None         # validated and uploaded once; needs the device, as the layers do

    # ---- bookkeeping: plain torch, any device ----
    def _view(self, buf, i):
        p, o = self.params[i], self.offsets[i]
        return buf[o:o + p.numel()].view(p.shape)

    def owns(self, params=None):
        """the parameters still live in the flat buffer"""
        params = self.params if params is None else list(params)
        base = self.flat.data_ptr()
        return len(params) == len(self.params) and all(p is q and p.data_ptr() == base + 4 * o for p, q, o in zip(params, self.params, self.offsets))

    def _collect_stray_gradients(self):
        """Detector.zero_grad() / a torch optimiser's zero_grad(set_to_none=True) detach p.grad from the flat buffer: the next backward then
        allocates fresh .grad tensors and the flat buffer would silently stay zero.  Copy such gradients in and re-attach the views (a missing
        .grad counts as zero, as in torch.optim) -- train_engine.FlatAdam's rule."""
        base = self.grad.data_ptr()
        for i, (p, o) in enumerate(zip(self.params, self.offsets)):
            g = p.grad
            if g is None or g.data_ptr() != base + 4 * o:
                view = self._view(self.grad, i)
                if g is None:
                    view.zero_()
                else:
                    view.copy_(g)
                p.grad = view

    def zero_grad(self, set_to_none=False):
        """zeroes the flat gradient and re-attaches the views (set_to_none is accepted and ignored: the views ARE the gradient)"""
        self.grad.zero_()
        base = self.grad.data_ptr()
        for i, (p, o) in enumerate(zip(self.params, self.offsets)):
            if p.grad is None or p.grad.data_ptr() != base + 4 * o:
                p.grad = self._view(self.grad, i)

    def state_dict(self):
        """the momentum buffer (None before it exists or without momentum), the step count and the settings"""
        return {'momentum_buffer': None if self.momentum_buffer is None or self.step_count == 0 else self.momentum_buffer.detach().cpu().clone(),
                'step_count': int(self.step_count), 'lr': float(self.param_groups[0]['lr']), 'momentum': self.momentum, 'weight_decay': self.weight_decay}

    def load_state_dict(self, state):
        buf = state['momentum_buffer']
        if buf is not None:
            if self.momentum_buffer is None or tuple(buf.shape) != tuple(self.momentum_buffer.shape):
                raise ValueError(f'FlatSGD.load_state_dict: a momentum buffer of {tuple(buf.shape)} does not fit this optimiser '
                                 f'({None if self.momentum_buffer is None else tuple(self.momentum_buffer.shape)})')
            self.momentum_buffer.copy_(buf)
        self.step_count = int(state['step_count']) if buf is not None or self.momentum_buffer is None else 0
        self.param_groups[0]['lr'] = float(state['lr'])

    # ---- the step: the device ----
    def step(self):
        """-> the total gradient norm (device scalar).  norm, update, one launch for every layer's packings; then every parameter's _version moves
        (the kernels wrote through raw pointers) and every layer records the versions it was packed at: the next forward packs nothing."""
        from .train_engine import _bump_version, _workspace
        if not self.flat.is_cuda:
            raise _lib.CosyHipError('FlatSGD.step runs on a ROCm device only (the parameters live on the CPU); there is no CPU fallback')
        if not self.owns():
            raise RuntimeError('FlatSGD.step: a parameter no longer lives in the flat buffer (.data was replaced): build the optimiser again')
        self._collect_stray_gradients()
        L, n, dev = _lib.lib(), self.flat.numel(), self.flat.device
        with torch.cuda.device(dev):
            s = _lib.stream()
            _lib.check(L.cosy_grad_norm_clip(_lib.ptr(self.grad), n, 0.0, _lib.ptr(self.norm_coef), _lib.ptr(_workspace(dev)), s))
            _lib.check(L.cosy_sgd_step(_lib.ptr(self.flat), _lib.ptr(self.grad), _lib.ptr(self.momentum_buffer), n, float(self.param_groups[0]['lr']),
                                       self.momentum, self.weight_decay, int(self.step_count == 0), s))
        self.step_count += 1
        if self.table is not None:
            self.table.run()
        for p in self.params:
            _bump_version(p)
        for layer in self.layers:              # after the bumps: what refresh() will compare against
            layer.versions = tuple((p._version, p.data_ptr()) for p in layer.parameters())
            layer.counter[0] += 1
        return self.norm_coef[0]
