#!/usr/bin/env python3
"""Count the instructions of the ADD-S inner loop of eval_tiles_kernel (cosypose_amd/csrc/kernels_eval.hip) in the device assembly
hipcc writes with the library's own flags, and record them in profiles/eval_isa.json next to the hash of the source: bench_eval.py
turns the count into the kernel's VALU-issue floor.  Run where the library is built:   python profiles/exp/eval_isa_count.py
"""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
from cosypose_amd import build as hipbuild   # noqa: E402

SRC = os.path.join(hipbuild.CSRC, 'kernels_eval.hip')


def main():
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [hipbuild.HIPCC] + hipbuild.FLAGS + hipbuild.FILE_FLAGS.get('kernels_eval.hip', []) + ['-c', SRC, '-o', os.path.join(tmp, 'e.o'), '-save-temps=obj']
        subprocess.run(cmd, check=True, capture_output=True)
        asm = open(os.path.join(tmp, 'kernels_eval-hip-amdgcn-amd-amdhsa-gfx950.s')).read()
    body = asm[asm.index('eval_tiles_kernel'):]
    body = body[:body.index('.end_amdhsa_kernel')] if '.end_amdhsa_kernel' in body else body
    best = None
    blocks = re.split(r'^(\.LBB\d+_\d+):.*$', body, flags=re.M)                    # [head, label, text, label, text, ...]
    for label, text in zip(blocks[1::2], blocks[2::2]):
        if not re.search(r'^\s*s_cbranch_\w+ ' + re.escape(label) + r'$', text, flags=re.M):
            continue                                                                # not a block that branches back to its own label
        ops = [l.split()[0] for l in text.split('\n') if l.strip() and not l.strip().startswith((';', '.'))]
        valu = [o for o in ops if o.startswith('v_')]
        if best is None or len(valu) > len(best['valu']):
            best = dict(label=label, ops=ops, valu=valu)
    assert best, 'no self-loop found in eval_tiles_kernel'
    reads = [o for o in best['ops'] if o.startswith('ds_read')]
    g = int(re.search(r'constexpr int EVAL_G = (\d+);', open(SRC).read()).group(1))
    pairs = len(reads) * g
    kinds = {}
    for o in best['valu']:
        kinds[o] = kinds.get(o, 0) + 1
    out = dict(kernel='eval_tiles_kernel', loop=best['label'], src_sha=hashlib.sha256(open(SRC, 'rb').read()).hexdigest()[:16],
               valu_per_iteration=len(best['valu']), lds_reads_per_iteration=len(reads), lds_read=sorted(set(reads)),
               salu_per_iteration=len([o for o in best['ops'] if o.startswith('s_')]), pairs_per_iteration=pairs,
               valu_per_pair=round(len(best['valu']) / pairs, 4), valu_kinds=kinds,
               hipcc=subprocess.run([hipbuild.HIPCC, '--version'], capture_output=True, text=True).stdout.strip().split('\n')[:2])
    json.dump(out, open(os.path.join(REPO, 'profiles', 'eval_isa.json'), 'w'), indent=1, sort_keys=True)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
