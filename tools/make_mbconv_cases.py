"""Rewrites the generated block of tests/_mbconv_cases.py (between its `# CASES-BEGIN` and `# CASES-END` lines: CLASS_COUNTS and
CASES) in place: for every fused-MBConv class the d0 ... d5 backbones use, the cheapest problem (B * Ho * Wo * mid, then H + W) with
the block's own Cin / mid / k / s whose plan has that class; then, per (dtype, form), problems that carry the edge geometries of
_mbconv_cases.EDGES (jointly where one problem can).  Host only: asks effdet_mbconv_plan_describe.

    python tools/make_mbconv_cases.py                  # regenerate the table
    python tools/make_mbconv_cases.py --old-coverage   # classes the hand-written shape lists of the three older kernel-level
                                                       # MBConv tests reach (the figures DESIGN.md quotes)
"""
import collections
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

import torch  # noqa: F401,E402  (one shared HIP runtime, see _lib.load)
import _mbconv_cases as mc  # noqa: E402
from ood_object_detection_amd import _lib  # noqa: E402

H_MAX, W_MAX = 200, 200


def search(lib, cfgs, dtype, gated, pred, small=False):
    """cheapest (cost, H + W) problem over the block configurations cfgs = {(Cin, mid, k, s)} and mc.floor(k) <= H, W <= MAX
    (small: mc.SMALLEST <= H, W - for the classes that only maps smaller than 2k + 1 reach, which the backbones run at 128 ... 384 px)"""
    best = None
    for Cin, mid, k, s in sorted(cfgs):
        lo = mc.SMALLEST if small else mc.floor(k)
        for H in range(lo, H_MAX + 1):
            Ho = mc.same_out(H, s)
            if best and mc.B * Ho * mc.same_out(lo, s) * mid > best[0][0]:
                break
            for W in range(lo, W_MAX + 1):
                cost = (mc.B * Ho * mc.same_out(W, s) * mid, H + W, Cin)
                if cost[0] > mc.MAX_ELEMS or (best and cost >= best[0]):
                    break
                case = (dtype, gated, Cin, mid, H, W, k, s)
                p = mc.case_plan(lib, case)
                if pred(p, case):
                    best = (cost, case, p)
                    break
    return best


def main():
    lib = _lib.load()
    used = mc.used_classes(lib)
    by_class = {}
    for blk in mc.swept_blocks():
        dt, gated, Cin, mid, H, W, k, s = blk[2:]
        c = mc.klass(mc.plan(lib, dt, gated, Cin, mid, H, W, k, s), dt, gated, k, s)
        by_class.setdefault(c, set()).add((Cin, mid, k, s))
    lines = []
    for c in sorted(used):
        pred = lambda p, case: mc.klass(p, case[0], case[1], case[6], case[7]) == c      # noqa: E731
        hit = search(lib, by_class[c], c[0], c[1], pred) or search(lib, by_class[c], c[0], c[1], pred, small=True)
        assert hit, c
        lines.append((hit[1], c, ()))
    for dt, form in sorted({(c[0], c[2]) for c in used}):
        cfgs = set().union(*[v for c, v in by_class.items() if (c[0], c[1], c[2]) == (dt, 0, form)])
        names = [e[0] for e in mc.EDGES if e[1](form)]
        holds = {e[0]: e[2] for e in mc.EDGES}
        for combo in (names[:-2] + names[-1:], names[:-3] + names[-2:-1]):     # (ragged ..., odd, s2 odd) and (ragged ..., s2 even)
            hit = search(lib, cfgs, dt, 0, lambda p, case: p['form'] == form and all(holds[n](p, case) for n in combo))
            if hit:
                lines.append((hit[1], mc.klass(hit[2], dt, 0, hit[1][6], hit[1][7]), tuple(combo)))
                continue
            for n in combo:
                hit = search(lib, cfgs, dt, 0, lambda p, case: p['form'] == form and holds[n](p, case))
                if hit:
                    lines.append((hit[1], mc.klass(hit[2], dt, 0, hit[1][6], hit[1][7]), (n,)))
                else:
                    print('# not reachable: %s %s: %s' % (mc.DTYPE_NAME[dt], mc.FORM_NAME[form], n))
    seen, rows = set(), []
    for case, c, edges in lines:
        if (case, edges) not in seen:
            seen.add((case, edges))
            rows.append('    (%s, %r, %r),\n' % (', '.join('%d' % v for v in case), c, edges))
    counts = collections.Counter((c[0], c[2]) for c in used)
    names = {mc.ROLL: 'ROLL', mc.WIDE: 'WIDE', mc.DEEP: 'DEEP', mc.FRONT: 'FRONT'}
    block = ('# classes per (dtype, form) that the sweep of swept_blocks() finds (recorded in DESIGN.md; the host test recounts them)\n'
             'CLASS_COUNTS = {%s}\n\n# fmt: off\nCASES = [\n%s]\n# fmt: on\n'
             % (', '.join('(%d, %s): %d' % (dt, names[f], n) for (dt, f), n in sorted(counts.items())), ''.join(rows)))
    path = os.path.join(ROOT, 'tests', '_mbconv_cases.py')
    with open(path) as f:
        src = f.read()
    head, rest = src.split('# CASES-BEGIN\n')
    tail = rest.split('# CASES-END\n')[1]
    with open(path, 'w') as f:
        f.write(head + '# CASES-BEGIN\n' + block + '# CASES-END\n' + tail)
    print('%d classes, %d cases written to %s' % (len(used), len(rows), path))


def old_coverage():
    """classes of the backbones that the parametrize lists of test_mbconv_expand_dw_fused / _gated (float32 and bf16) and
    test_mbconv_expand_dw_pair (two-term bf16) reach, per (dtype, form)"""
    import test_accurate_gpu
    import test_kernels_gpu
    lib = _lib.load()
    used = mc.used_classes(lib)

    def shapes(fn):
        return [a for m in fn.pytestmark if m.name == 'parametrize' and 'Cin' in m.args[0] for a in m.args[1]]
    reached = set()
    for dt in (0, 1):
        for gated, fn in ((0, test_kernels_gpu.test_mbconv_expand_dw_fused), (1, test_kernels_gpu.test_mbconv_expand_dw_gated)):
            for Cin, mid, H, W, k, s in shapes(fn):
                reached.add(mc.klass(mc.plan(lib, dt, gated, Cin, mid, H, W, k, s), dt, gated, k, s))
    for Cin, mid, H, W, k, s, gated in shapes(test_accurate_gpu.test_mbconv_expand_dw_pair):
        reached.add(mc.klass(mc.plan(lib, 2, gated, Cin, mid, H, W, k, s), 2, int(gated), k, s))
    tot = collections.Counter((c[0], c[2]) for c in used)
    hit = collections.Counter((c[0], c[2]) for c in used if c in reached)
    for key in sorted(tot):
        print('%-14s %-5s %3d classes, %3d reached by the older tests' % (mc.DTYPE_NAME[key[0]], mc.FORM_NAME[key[1]], tot[key], hit[key]))
    print('total %d, reached %d' % (sum(tot.values()), sum(hit.values())))


if __name__ == '__main__':
    old_coverage() if '--old-coverage' in sys.argv[1:] else main()
