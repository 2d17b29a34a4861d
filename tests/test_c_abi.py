"""The boundary between include/cosyhip.h and its Python side, checked by the C compiler (CPU only).

The header is the declaration.  cosypose_amd/_lib.py reads every entry point's signature from it; the structs and constants that Python
restates (ctypes.Structure classes, numpy record dtypes, plain integers) are compared here, field by field and value by value, with what a
C99 program that includes the header prints.  A new struct mirror needs one line in MIRRORS, a new constant one line in constants().
"""
import ctypes
import os
import pathlib
import re
import subprocess

import pytest
import torch

from cosypose_amd import _lib
from cosypose_amd.build import HEADER, LIB, build

def _mirrors():
    from cosypose_amd import augmentations, detector_input, frames, model_info, resize
    # C type, its Python mirror, the C field names in declaration order (`c=py` where Python has to spell a name differently)
    return [
        ('cosy_prof_rec_t', _lib.ProfRec, 'name layer n ms_avg ms_min bytes flops cbytes'),
        ('cosy_mesh_t', _lib.MeshSet, 'verts colors normals uvs tex faces n_faces V F TH TW'),
        ('cosy_shade_t', _lib.Shade, 'ambient diffuse specular shininess light light_frame smooth quantize'),
        ('cosy_ba_ctrl_t', _lib.BaCtrl, 'loss next_loss lambda=lambd done prev_update finished n_hist'),
        ('cosy_ba_batch_t', _lib.BaBatch, 'G n_cand n_obj n_views n_mesh P S max_blocks n_hist_rows optimize_cameras a_total residuals_threshold L_down L_up '
         'eps table cand_TCO K pts_table sym_table n_sym TWO_9d TCW_9d TWO_9d_updated TCW_9d_updated ctrl hist_iteration hist_lambda hist_loss '
         'hist_TWO_9d hist_TCW_9d workspace'),
        ('cosy_aug_params_t', augmentations.PARAMS_DTYPE, 'bg flags k sharpness contrast brightness color reserved'),
        ('cosy_model_info_t', model_info.RECORD, 's_max min max i j n_bad'),
        ('cosy_resize_item_t', resize.ITEM_DTYPE, 'src h w hb hk hks vb vk vks'),
        ('cosy_frame_item_t', frames.ITEM_DTYPE, 'image mask h w xb yb xn yn'),
        ('cosy_rpn_levels_t', _lib.RpnLevels, 'objectness deltas H W stride_h stride_w base'),
        ('cosy_msroi_levels_t', _lib.MsroiLevels, 'feat H W scale'),
        ('cosy_detin_item_t', detector_input.ITEM_DTYPE, 'frame sc sy sx masks masks_out boxes boxes_out h w nh nw xb yb xn yn n_masks n_boxes rw rh flags '
         'reserved'),
        ('cosy_head_layer_t', _lib.HeadLayer, 'x w bias out out1 dtype ksize c_in c_out relu store n_split n_levels row_start H W'),
    ]


MIRRORS = [(ctype, mirror, [(f.split('=')[0], f.split('=')[-1]) for f in fields.split()]) for ctype, mirror, fields in _mirrors()]      # (C name, Python name)


def constants():
    """header name -> every Python spelling of it"""
    from cosypose_amd import augmentations as aug, detector, detector_heads, detector_input, detector_rpn, detector_train, resize
    return {
        'COSY_F32': [_lib.COSY_F32, _lib.DTYPES[torch.float32]],
        'COSY_BF16': [_lib.COSY_BF16, _lib.DTYPES[torch.bfloat16]],
        'COSY_F16': [_lib.COSY_F16, _lib.DTYPES[torch.float16]],
        'COSY_MASK_U8': [_lib.COSY_MASK_U8], 'COSY_MASK_I32': [_lib.COSY_MASK_I32],
        'COSY_HEAD_STORE_ROWS': [_lib.HEAD_STORE_ROWS], 'COSY_HEAD_STORE_NCHW': [_lib.HEAD_STORE_NCHW],
        'COSY_HEAD_STORE_DECONV_ROWS': [_lib.HEAD_STORE_DECONV_ROWS], 'COSY_HEAD_STORE_DECONV_NCHW': [_lib.HEAD_STORE_DECONV_NCHW],
        'COSY_RPN_MAX_LEVELS': [_lib.RPN_MAX_LEVELS, detector_rpn.MAX_LEVELS, detector_heads.MAX_LEVELS],
        'COSY_RPN_MAX_ANCHORS': [_lib.RPN_MAX_ANCHORS, detector_rpn.MAX_ANCHORS_PER_CELL],
        'COSY_AUG_GATE': [_lib.AUG_GATE, aug.GATE], 'COSY_AUG_SHARPNESS': [_lib.AUG_SHARPNESS, aug.SHARPNESS],
        'COSY_AUG_CONTRAST': [_lib.AUG_CONTRAST, aug.CONTRAST], 'COSY_AUG_BRIGHTNESS': [_lib.AUG_BRIGHTNESS, aug.BRIGHTNESS],
        'COSY_AUG_COLOR': [_lib.AUG_COLOR, aug.COLOR], 'COSY_AUG_GRAY': [_lib.AUG_GRAY, aug.GRAY],
        'COSY_RESIZE_BILINEAR': [_lib.RESIZE_BILINEAR, resize.FILTERS['bilinear']],
        'COSY_RESIZE_BICUBIC': [_lib.RESIZE_BICUBIC, resize.FILTERS['bicubic']],
        'COSY_DT_MAX_GT': [_lib.DT_MAX_GT, detector_train.MAX_GT], 'COSY_DT_MAX_BATCH': [_lib.DT_MAX_BATCH, detector_train.MAX_BATCH],
        'COSY_DT_MAX_M': [_lib.DT_MAX_M, detector_train.MAX_MASK_SIDE],
        'COSY_DT_MAX_CLASSES': [_lib.DT_MAX_CLASSES, detector.MAX_CLASSES, detector_train.MAX_CLASSES],
        'COSY_DETIN_ONE_TAP': [_lib.DETIN_ONE_TAP, detector_input.ONE_TAP],
    }


@pytest.fixture(scope='module')
def probe(tmp_path_factory):
    """what the C compiler makes of the header: {'sizeof': {type: bytes}, 'field': {(type, field): (offset, bytes)}, 'const': {name: value}}"""
    body = []
    for ctype, _, fields in MIRRORS:
        body.append(f'    printf("sizeof {ctype} - %zu 0\\n", sizeof({ctype}));')
        body += [f'    printf("field {ctype} {c} %zu %zu\\n", offsetof({ctype}, {c}), sizeof((({ctype}*)0)->{c}));' for c, _ in fields]
    body += [f'    printf("const {name} - %lld 0\\n", (long long)({name}));' for name in constants()]
    d = tmp_path_factory.mktemp('c_abi')
    (d / 'probe.c').write_text('#include <stddef.h>\n#include <stdio.h>\n#include "cosyhip.h"\nint main(void) {\n' + '\n'.join(body) + '\n    return 0;\n}\n')
    cc = subprocess.run([os.environ.get('CC', 'cc'), '-std=c99', '-Wall', '-Werror', '-I', os.path.dirname(HEADER), str(d / 'probe.c'), '-o', str(d / 'probe')],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    out = {'sizeof': {}, 'field': {}, 'const': {}}
    for kind, a, b, x, y in (line.split() for line in subprocess.run([str(d / 'probe')], capture_output=True, text=True, check=True).stdout.splitlines()):
        out[kind][(a, b) if kind == 'field' else a] = (int(x), int(y)) if kind == 'field' else int(x)
    return out


@pytest.mark.parametrize('ctype,mirror,fields', MIRRORS, ids=[m[0] for m in MIRRORS])
def test_struct_mirror_has_the_headers_layout(probe, ctype, mirror, fields):
    if isinstance(mirror, type) and issubclass(mirror, ctypes.Structure):
        names, size = [n for n, *_ in mirror._fields_], ctypes.sizeof(mirror)
        layout = {n: (getattr(mirror, n).offset, getattr(mirror, n).size) for n in names}
    else:
        names, size = list(mirror.names), mirror.itemsize
        layout = {n: (mirror.fields[n][1], mirror.fields[n][0].itemsize) for n in names}
    assert names == [py for _, py in fields], f'{ctype}: the mirror\'s fields {names} are not the header\'s, in its order'
    for c, py in fields:
        assert layout[py] == probe['field'][ctype, c], f'{ctype}.{c}: mirror (offset, size) {layout[py]}, header {probe["field"][ctype, c]}'
    assert size == probe['sizeof'][ctype], f'{ctype}: mirror {size} bytes, header {probe["sizeof"][ctype]}'


def test_every_struct_of_the_header_has_a_checked_mirror():
    code = re.sub(r'/\*.*?\*/', '', pathlib.Path(HEADER).read_text(), flags=re.S)
    assert sorted(re.findall(r'\}\s*(cosy_\w+_t)\s*;', code)) == sorted(m[0] for m in MIRRORS)


def test_constants_have_the_headers_values(probe):
    for name, spellings in constants().items():
        for value in spellings:
            assert value == probe['const'][name], f'{name}: Python {value}, header {probe["const"][name]}'


_P, _I, _F, _D, _L, _LL, _SZ = (ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_long, ctypes.c_longlong, ctypes.c_size_t)
PINNED = {      # written out by hand from the header; between them: every scalar type, T**, T* const*, struct pointers, (void), const char*
    'cosy_version': ([], _I),
    'cosy_last_error': ([], ctypes.c_char_p),
    'cosy_effnet_b3_param_count': ([], _L),
    'cosy_effnet_b3_create': ([_P, _SZ, _I, _I, _I, _I, _P], _I),
    'cosy_crop_geometry': ([_P, _P, _P, _P, _P, _I, _I, _F, _I, _I, _I, _I, _F, _P, _P, _P, _P], _I),
    'cosy_bn_train_stats': ([_P, _L, _I, _F, _F, _P, _P, _P, _P, _P, _P], _I),
    'cosy_ba_linearize': ([_P] * 6 + [_I] * 5 + [_D] + [_P] * 8, _I),
    'cosy_ba_batch_workspace_bytes': ([_I, _I, _LL], _SZ),
    'cosy_train_gemm_packed': ([_P, _P, _LL, _L, _I, _I, _P, _P, _P], _I),
    'cosy_msroi_align_backward': ([_P, _P, _I, _I, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P], _I),
    'cosy_detector_input': ([_P, _P, _I, _I, _I, _P, _L, _I, _I, _I, _P, _P], _I),
    'cosy_head_conv': ([_P, _P], _I),
}


@pytest.mark.parametrize('name', PINNED)
def test_derived_signature_equals_the_hand_written_one(name):
    assert _lib._SIGNATURES[name] == PINNED[name], f'{name}: derived {_lib._SIGNATURES[name]}'


def test_parser_on_synthetic_headers():
    parse = _lib.parse_header
    assert parse('''
        /* cosy_x(int a); is only mentioned here; */
        #define COSY_N (1 << 4)
        typedef struct { int a[COSY_N]; float *p, *q; } cosy_s_t;
        int
        cosy_three_lines(const cosy_s_t* s, long long n,   /* a comment, with a comma, inside */
                         unsigned flags,
                         double tol, cosy_stream_t stream);
        size_t cosy_array(const float m[9], float* const* rows, unsigned long long* mask, size_t bytes);   // cosy_y(int);
        const char* cosy_text(void);
        long cosy_empty();
    ''') == {'cosy_three_lines': ([_P, _LL, ctypes.c_uint, _D, _P], _I), 'cosy_array': ([_P, _P, _P, _SZ], _SZ),
             'cosy_text': ([], ctypes.c_char_p), 'cosy_empty': ([], _L)}
    for bad in ('int cosy_bad_arg(int n, short k);', 'void cosy_bad_ret(int n);', 'float* cosy_bad_ptr(void);', 'int cosy_bad_struct(cosy_s_t by_value);'):
        with pytest.raises(_lib.CosyHipError, match=re.search(r'cosy_bad_\w+', bad).group()):
            parse(bad)


def test_header_library_and_exports_name_the_same_entry_points():
    build()
    code = re.sub(r'/\*.*?\*/', '', pathlib.Path(HEADER).read_text(), flags=re.S)
    declared = set(re.findall(r'\b(cosy_[a-z0-9_]+)\s*\(', code))
    nm = subprocess.run(['nm', '-D', '--defined-only', LIB], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.split()[-1].startswith('cosy_')}
    assert declared == set(_lib.EXPORTS) == exported, (declared ^ set(_lib.EXPORTS), declared ^ exported)
    assert len(_lib.EXPORTS) == len(declared)          # header order, every name once
    lib = ctypes.CDLL(LIB)
    assert all(hasattr(lib, name) for name in declared)
