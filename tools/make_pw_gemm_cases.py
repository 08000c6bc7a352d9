"""Rewrites the generated block of tests/_pw_gemm_cases.py (between its `# CASES-BEGIN` and `# CASES-END` lines) in place: for
every class of the 1x1-conv GEMM that the d0 ... d5 networks, MetaHead and ProjectionNet use and that no named case reaches, the
smallest case that reaches it - the N of the call that uses the class, the smallest K with its stage-count class and K tail, and
three images of 150 rows (the small form) or 512 workgroups of 34 rows each (the large form: both pixel tiles of the first
wave and two rows of the second; all four waves of the large form run in the named project-conv cases).  The classes of the group
launch are packed, up to eight problems to a launch.  The forms are asked of the library's plan queries.  Host only.

    python tools/make_pw_gemm_cases.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

import torch  # noqa: F401,E402  (one shared HIP runtime, see _lib.load)
import _pw_gemm_cases as pc  # noqa: E402
from ood_object_detection_amd import _lib  # noqa: E402

LIMIT = 64 << 20                              # bytes of a case's A, W or output


def smallest_k(lib, c, N):
    dt, group = c[0], c[7]
    for K in range(8, 8192, 8):
        p = pc.group_plan(lib, dt, [(150, K, N)]) if group else pc.plan(lib, dt, 150, K, N, 150, c[3], c[4])
        if pc.klass(dt, p, K, c[4], c[5], group)[8:] == c[8:]:
            return K
    raise AssertionError(c)


def single_case(lib, name, c, use):
    dt, BN, PT, gated, res, act, vec, group, nstc, tail = c
    N = use[2][4]
    K = smallest_k(lib, c, N)
    n_tiles = pc.plan(lib, dt, 150, K, N)['n_tiles']
    B, rpi = ((512 + n_tiles - 1) // n_tiles, 34) if PT == 2 and BN != 128 else (3, 150)
    case = (name, dt, B, rpi, K, N, bool(gated), bool(res), act, not (N == pc.ANCHORS or act == 2), 'dense')
    es = 2 if dt == 1 else 4
    assert max(B * rpi * K, N * K, B * rpi * N) * es <= LIMIT, case
    return case


def group_case(lib, name, classes, used):
    """up to eight classes of one dtype, tile, form and act in one launch: a problem per class, each with the class's smallest K;
    the last problem has no scale; a lone class gets a second problem beside it"""
    dt, BN, PT, _, _, act = classes[0][:6]
    N = used[classes[0]][2][2][0][2]
    ks = [smallest_k(lib, c, N) for c in classes] + ([24] if len(classes) == 1 else [])
    n = len(ks)
    rows = [((512 + n - 1) // n - 1) * 128 + 2 + i for i in range(n)] if PT == 2 else [150 - 9 * i for i in range(n)]
    return (name, dt, tuple((M, K, N, i + 1 < n) for i, (M, K) in enumerate(zip(rows, ks))), act)


def main():
    lib = _lib.load()
    used = pc.used_classes(lib)
    have = set()
    for case in pc.NAMED:
        have.update(pc.case_classes(lib, case) or [])
    todo = [c for c in sorted(used, key=repr) if c not in have]
    single, groups = [], []
    for c in todo:
        if not c[7]:
            single.append(single_case(lib, 'form%03d' % len(single), c, used[c]))
    packs = {}
    for c in todo:
        if c[7]:
            packs.setdefault(c[:8] + (used[c][2][2][0][2],), []).append(c)
    for key in sorted(packs, key=repr):
        for i in range(0, len(packs[key]), 8):
            groups.append(group_case(lib, 'form%03d' % (len(single) + len(groups)), packs[key][i:i + 8], used))
    for case in single + groups:
        have.update(pc.case_classes(lib, case))
    assert not [c for c in used if c not in have]
    lines = ['# fmt: off', 'FORM_CASES = ['] + ['    %r,' % (c,) for c in single] + [']', 'FORM_GROUP_CASES = [']
    lines += ['    %r,' % (c,) for c in groups] + [']', '# fmt: on']
    path = os.path.join(ROOT, 'tests', '_pw_gemm_cases.py')
    src = open(path).read()
    head, rest = src.split('# CASES-BEGIN\n')
    _, tail = rest.split('# CASES-END')
    open(path, 'w').write(head + '# CASES-BEGIN\n' + '\n'.join(lines) + '\n# CASES-END' + tail)
    print('%d used classes, %d generated single cases, %d generated group cases' % (len(used), len(single), len(groups)))


if __name__ == '__main__':
    main()
