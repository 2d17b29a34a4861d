"""The detector backward's entry points come in pairs, float32 rows and bfloat16 rows (`16`), and each pair runs ONE validator
(csrc/detbwd_device.h, csrc/kernels_detbwd.hip): the same invalid call is refused by both with the same words after the entry's own name.
The pack table (cosy_pack_table_build) refuses a bad row in the words of the per-layer packs.  No call here launches a kernel."""
import ctypes

import pytest
import torch

from cosypose_amd import _lib

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
C, O, B, H, W = 8, 16, 1, 4, 4                 # a 3x3 layer of C -> O channels on one 4 x 4 map
ROOM = 1 << 16                                 # elements of every buffer: more than any call here could touch if it were accepted


def _tail(entry, rc, word):
    """the message of a refused call without the entry's own name; it must be the refusal of the rule under test"""
    msg = _lib.lib().cosy_last_error().decode()
    assert rc == -1 and msg.startswith(entry + ': '), (entry, rc, msg)
    assert word in msg, (entry, word, msg)
    return msg[len(entry) + 2:]


def test_backward_entry_refusals_agree():
    L = _lib.lib()
    buf = {dt: {k: torch.zeros(ROOM, dtype=dt, device='cuda') for k in ('x', 'g', 'w', 'out', 'y')} for dt in (F32, BF16)}
    dw, db, dw1, db1, ws = (torch.zeros(ROOM, device='cuda') for _ in range(5))
    need = int(L.cosy_head_wgrad_workspace_bytes(B * H * W, 3, C, O))
    assert 0 < need <= 4 * ROOM

    def desc(dt, grad, **kw):
        """the weight gradient's descriptor (x: rows of C channels), or the data gradient's (x: the rows g of O channels, out: C channels)"""
        d = _lib.HeadLayer()
        b = buf[dt]
        d.x, d.w, d.out = (_lib.ptr(b['g']), _lib.ptr(b['w']), _lib.ptr(b['out'])) if grad == 'd' else (_lib.ptr(b['x']), None, None)
        d.dtype, d.ksize, d.relu, d.store, d.n_levels = _lib.DTYPES[dt], 3, 0, _lib.HEAD_STORE_ROWS, 1
        d.c_in, d.c_out = (O, C) if grad == 'd' else (C, O)
        d.n_split = d.c_out
        d.row_start[0], d.row_start[1], d.H[0], d.W[0] = 0, B * H * W, H, W
        for k, v in kw.items():
            if k in ('row_start', 'H', 'W'):
                for i, n in v.items():
                    getattr(d, k)[i] = n
            else:
                setattr(d, k, v)
        return d

    def call(family, dt, change, stride=1, y=False, nbytes=need, null_dw=False):
        d = desc(dt, family[-5], **change)                                       # 'd' or 'w' of ..._dgrad / ..._wgrad
        entry = family + ('' if dt == F32 else '16')
        fn, b, s = getattr(L, entry), buf[dt], _lib.stream()
        yp = _lib.ptr(b['y']) if y else None
        p_dw = None if null_dw else _lib.ptr(dw)
        if family == 'cosy_head_dgrad':
            return entry, fn(ctypes.byref(d), yp, s)
        if family == 'cosy_trunk_dgrad':
            return entry, fn(ctypes.byref(d), stride, None, 0, 0, 0, None, 0, 0, 0, yp, s)
        if family == 'cosy_head_wgrad':
            return entry, fn(ctypes.byref(d), _lib.ptr(b['g']), p_dw, _lib.ptr(db), _lib.ptr(dw1), _lib.ptr(db1), _lib.ptr(ws), nbytes, s)
        return entry, fn(ctypes.byref(d), stride, _lib.ptr(b['g']), None, p_dw, _lib.ptr(db), _lib.ptr(ws), nbytes, s)

    ALL = ('cosy_head_dgrad', 'cosy_trunk_dgrad', 'cosy_head_wgrad', 'cosy_trunk_wgrad')
    WGRAD, TRUNK = ALL[2:], (ALL[1], ALL[3])
    two_levels = dict(n_levels=2, row_start={2: 2 * B * H * W}, H={1: H}, W={1: W})
    too_many = dict(row_start={1: (1 << 30) + 1}, H={0: 1}, W={0: 1})
    cases = [                                                                    # (families, the word of the rule, the change, how it is called)
        (ALL, 'ksize', dict(ksize=5), {}),
        (ALL, 'c_in=12', dict(c_in=12), {}),
        (ALL, 'c_out=0', dict(c_out=0, n_split=0), {}),
        (ALL[2:3], 'n_split', dict(n_split=0), {}),
        (ALL[2:3], 'n_split', dict(n_split=O + 1), {}),
        (TRUNK, 'one level', two_levels, dict(stride=2)),
        (ALL, 'row_start[0]', dict(row_start={0: 4}), {}),
        (ALL, '2^30', too_many, {}),
        (WGRAD, 'workspace_bytes', {}, dict(nbytes=need - 4)),
        (WGRAD, 'null dw0', {}, dict(null_dw=True)),
        (ALL[0:1], 'no y', dict(store=_lib.HEAD_STORE_NCHW), dict(y=True)),
    ]
    for families, word, change, how in cases:
        for family in families:
            tails = [_tail(*call(family, dt, change, **how), word) for dt in (F32, BF16)]
            assert tails[0] == tails[1], (family, word, tails)
    assert call('cosy_head_dgrad', F32, dict(row_start={1: 0}))[1] == 0           # the descriptors are valid but for the change: M = 0 is accepted
    assert call('cosy_trunk_dgrad', BF16, dict(row_start={1: 0}))[1] == 0

    # the packs: both heads' entries, both trunk's entries and a row of the pack table run check_weight_pack
    wp, bp, fwd, bias, bwd = (_lib.ptr(t) for t in (dw, db, buf[F32]['w'], db1, buf[F32]['out']))
    fwd16, bwd16 = _lib.ptr(buf[BF16]['w']), _lib.ptr(buf[BF16]['out'])
    table = torch.zeros(L.cosy_pack_table_bytes(1), dtype=torch.uint8, device='cuda')

    def head_pack(dt, **kw):
        a = dict(w0=wp, b0=bp, w1=None, b1=None, ksize=3, c_in=C, n0=O, n1=0, fwd=fwd if dt == F32 else fwd16, fwd_bias=bias, bwd=bwd if dt == F32 else bwd16)
        a.update(kw)
        entry = 'cosy_head_weight_pack' + ('' if dt == F32 else '16')
        return entry, getattr(L, entry)(*a.values(), _lib.stream())

    def trunk_pack(dt, **kw):
        a = dict(w=wp, scale=None, shift=bp, ksize=3, c_in=C, c_out=O, fwd=fwd if dt == F32 else fwd16, fwd_bias=bias, bwd=bwd if dt == F32 else bwd16)
        a.update(kw)
        entry = 'cosy_trunk_weight_pack' + ('' if dt == F32 else '16')
        return entry, getattr(L, entry)(*a.values(), _lib.stream())

    def table_row(dt, **kw):
        a = dict(w0=wp, b0=bp, w1=0, b1=0, scale=0, fwd=fwd if dt == F32 else fwd16, fwd_bias=bias, bwd=bwd if dt == F32 else bwd16, ksize=3, c_in=C, n0=O, n1=0,
                 dtype=_lib.DTYPES[dt])
        a.update({k: (0 if v is None else v) for k, v in kw.items()})
        n = ctypes.c_longlong(-1)
        rc = L.cosy_pack_table_build((ctypes.c_longlong * 13)(*a.values()), 1, _lib.ptr(table), table.numel(), ctypes.byref(n), _lib.stream())
        assert n.value == -1
        return 'cosy_pack_table_build: layer 0', rc

    for word, change, packs in (('null fwd', dict(fwd=None), (head_pack, trunk_pack, table_row)),
                                ('null w1 or b1', dict(n1=8), (head_pack, table_row)),
                                ('a deconvolution has no sibling', dict(ksize=2, n1=8, w1=wp, b1=bp), (head_pack, table_row)),
                                ('c_in=12', dict(c_in=12), (head_pack, trunk_pack, table_row))):
        tails = [_tail(*pack(dt, **change), word) for pack in packs for dt in (F32, BF16)]
        assert len(set(tails)) == 1, (word, tails)
    torch.cuda.synchronize()
