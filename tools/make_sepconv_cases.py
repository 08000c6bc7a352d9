"""Rewrites the generated block of tests/_sepconv_cases.py (between its `# CASES-BEGIN` and `# CASES-END` lines) in place: the
cases of the fused separable conv in float32, bf16 and bf16 with float32 outputs - every node kind, head layer, box predict,
AnchorNet layer and predict at every BiFPN width, the class predicts at the class counts that cut the 96- and 64-class chunks in
every way - each with the class the library's plan query (effdet_sepconv_plan_describe) gives it.  Host only.

    python tools/make_sepconv_cases.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

import torch  # noqa: F401,E402  (one shared HIP runtime, see _lib.load)
import _sepconv_cases as sc  # noqa: E402
from ood_object_detection_amd import _lib  # noqa: E402

# class counts of the class predicts per width: around one class, the 8-channel piece, the 32-channel group, the 96-class chunk
# (97 and 192: a last sub-chunk of one class / full sub-chunks) and the 64-class sub-chunk float32 takes at 288 (65 and 128), and
# everywhere the configurations' own 400 (five sub-chunks of 96, seven of 64)
CLASS_COUNTS = {64: (1, 2, 7, 90, 96, 97, 98, 150, 192, 400), 88: (1, 2, 7, 90, 96, 97, 98, 150, 192, 400),
                288: (1, 64, 65, 90, 97, 128, 192, 400)}
BETWEEN = (7, 90, 97, 192, 400)


def cases():
    out = []
    for dt in (0, 1):
        for F in sc.WIDTHS:
            for kind in sc.NODE_KINDS:
                out.append(('node', dt, F, F, 0, kind))
            for N in sorted({F, sc.ANCHOR_CH}):
                out.append(('layer', dt, F, N, 0, ''))
            out.append(('box', 3 if dt else 0, F, 4 * sc.A, 0, ''))
            for C in CLASS_COUNTS.get(F, BETWEEN):
                out.append(('cls', dt, F, sc.A * C, C, 'aligned'))
            if dt == 1:                                              # bf16: every general class-predict form with vec_ok off by the
                for C in (90, 192, 400):                             # image stride - one chunk per anchor, full and cut sub-chunks
                    out.append(('cls', dt, F, sc.A * C, C, 'odd'))
        out.append(('anchor', dt, sc.ANCHOR_CH, sc.A, 0, ''))
    return out


def main():
    lib = _lib.load()
    lines = ['# fmt: off', 'CASES = [']
    for c in cases():
        p = sc.case_plan(lib, c)
        assert p is not None, c
        lines.append('    %r,' % (c + (sc.klass(p),),))
    lines += [']', '# fmt: on']
    path = os.path.join(ROOT, 'tests', '_sepconv_cases.py')
    src = open(path).read()
    head, rest = src.split('# CASES-BEGIN\n')
    _, tail = rest.split('# CASES-END')
    open(path, 'w').write(head + '# CASES-BEGIN\n' + '\n'.join(lines) + '\n# CASES-END' + tail)
    print('%d cases, %d classes' % (len(lines) - 4, len({l.split(', (')[-1] for l in lines[2:-2]})))


if __name__ == '__main__':
    main()
