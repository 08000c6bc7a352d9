"""Rewrites the generated block of tests/_train_cases.py (between its `# CASES-BEGIN` and `# CASES-END` lines: CLASS_COUNTS and
CASES) in place: for every kernel class of the training GEMMs and depthwise entries that the d0 ... d5 training step uses
(_train_cases.swept_calls), the cheapest problem (largest operand or output, then the sum of the dimensions) whose own plan has
that class; then, per class, problems that carry the edges of _train_cases.*_EDGES that apply to it (jointly where one problem
can: _train_cases.*_COMBOS).  Host only: asks the effdet_train_*_plan_describe queries.

    python tools/make_train_cases.py                  # regenerate the table
    python tools/make_train_cases.py --old-coverage   # classes the hand-written shape lists of the six older kernel-level tests of
                                                      # tests/test_train_gpu.py reach (the figures DESIGN.md quotes)
"""
import collections
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    sys.path.insert(0, p)

import torch  # noqa: F401,E402  (one shared HIP runtime, see _lib.load)
import _train_cases as tc  # noqa: E402
from ood_object_detection_amd import _lib  # noqa: E402

# level geometries of the *_levels cases (B, ((h, w), ...)), and the candidate values of the searches
_HW = [((1, 1),), ((2, 2), (1, 1)), ((3, 2), (2, 1), (1, 1)), ((5, 4), (3, 2), (2, 1)), ((7, 6), (4, 3), (2, 2), (1, 1)),
       ((8, 8), (4, 4), (2, 2), (1, 1)), ((10, 6), (5, 3), (3, 2)), ((13, 11), (7, 6), (4, 3)), ((12, 12), (6, 6), (3, 3), (2, 2), (1, 1)),
       ((16, 16), (8, 8), (4, 4), (2, 2), (1, 1)), ((21, 19), (11, 10), (6, 5), (3, 3), (2, 2)), ((32, 32), (16, 16), (8, 8), (4, 4), (2, 2)),
       ((41, 37), (21, 19), (11, 10), (6, 5), (3, 3)), ((64, 64), (32, 32), (16, 16), (8, 8), (4, 4))]
LVS = [(B, hw) for hw in _HW for B in (1, 2, 3)]
# many row counts of a few thousand, for the classes whose slice count the rows decide
LVS_MANY = LVS + [(B, ((a, b), (3, 2), (1, 1))) for a in range(30, 120, 7) for b in (a, a - 3) for B in (1, 2, 3)]
NT_N = list(range(1, 24)) + list(range(65, 84))
NT_K = {1: list(range(1, 64)) + [64, 80], 4: list(range(384, 452))}
TN_N = list(range(1, 40)) + [100, 124, 126, 243, 250, 252] + list(range(256, 264)) + list(range(384, 392)) + [544, 546, 548, 549]
TN_K = list(range(1, 17)) + [20, 27, 28, 32, 60, 64, 124, 128, 132, 136, 192, 196, 252, 255, 256, 260, 380, 508, 511, 572, 576, 580]
DW_C = (4, 8, 68, 72, 132)
DW_B = (1, 2, 3)
DW_H = list(range(1, 72)) + [n + d for n in (683, 1025, 1366, 2049, 4097) for d in range(0, 4)]
DW_W = list(range(1, 132))
LIMIT = [tc.MAX_ELEMS]                                     # the element limit of the search that is running


def cost(call):
    dims = call[2:5] if call[0] != 'dw' else call[2:6]
    return (tc.elems(call), sum(dims))


def _ok(lib, call, cls, names):
    p = tc.plan(lib, call)
    if p is None or tc.klass(p, call) != cls:
        return False
    return all(tc.holds(n, p, call) for n in names)


def _forms(calls, idx):
    return sorted({tuple(c[i] for i in idx) for c in calls})


def search_nt(lib, cls, calls, names):
    """cheapest gemm_nt problem of class cls that carries the edges `names`, over the (entry, operands, alignment) forms of the swept
    calls of that class"""
    best = None
    need_m = any(n.startswith('M % 128') for n in names)
    for entry, akind, ckind, ops, align in _forms(calls, (1, 5, 6, 9, 11)):
        levels = tc.LEVELS in (akind, ckind)
        for N in NT_N:
            for K in NT_K[cls[2]]:
                cols = K if akind != tc.DENSE else N
                for ld in ((cols, cols + 2, cols + 4, cols + 8) if levels else (0,)):
                    if levels:
                        ms = [(tc.levels_rows(lv), lv) for lv in LVS]
                    else:
                        ms = [(M, None) for M in ((129, 130, 131, 132, 133, 140, 161, 162, 164) if need_m else (1, 2, 3, 4, 5, 31, 33, 40, 64))]
                    for M, lv in ms:
                        pk = (0, sum(h * w for h, w in lv[1]) * ld, ld) if levels else (0, 0, 0)
                        for rows in ((20, 24, M) if ops & tc.A_SCALE else (0,)):
                            if rows > M:
                                continue
                            call = ('nt', entry, M, K, N, akind, ckind, pk, lv, ops, rows, align)
                            c = cost(call)
                            if (best and c >= best[0]) or c[0] > LIMIT[0]:
                                continue
                            if _ok(lib, call, cls, names):
                                best = (c, call)
    return best and best[1]


def search_tn(lib, cls, calls, names):
    best = None
    forms = _forms(calls, (1, 5, 9))
    for entry, ykind, align in forms:
        levels = ykind == tc.LEVELS
        for N in TN_N:
            for K in TN_K:
                for ld in ((N, N + 2, N + 4) if levels else (0,)):
                    if levels:
                        ms = [(tc.levels_rows(lv), lv) for lv in (LVS_MANY if cls[7] == 2 else LVS)]
                    elif cls[7] == 2:                          # empty trailing slices: S is bounded by the tile count, not by the rows
                        p = tc.plan(lib, ('tn', entry, 1 << 20, N, K, ykind, (0, 0, 0), None, 0, align))
                        if p is None or p['S'] < 9 or p['S'] > 64:
                            continue
                        ms = [(M, None) for M in range(256 * (p['S'] - 1) + 1, 256 * p['S'] + 800)]
                    else:
                        ms = [(M, None) for M in (list(range(1, 70)) if cls[7] == 0 else list(range(257, 330)))]
                    for M, lv in ms:
                        pk = (0, sum(h * w for h, w in lv[1]) * ld, ld) if levels else (0, 0, 0)
                        c = cost(('tn', entry, M, N, K, ykind, pk, lv, 0, align))
                        if c[0] > LIMIT[0] or (best and c >= best[0]):
                            if not levels:
                                break                          # M ascends: nothing cheaper follows
                            continue
                        for rows in ((5, 9, 24, M) if entry == 'gemm_tn_scaled' else (0,)):
                            call = ('tn', entry, M, N, K, ykind, pk, lv, rows, align)
                            if rows <= M and _ok(lib, call, cls, names):
                                best = (c, call)
                                break
    return best and best[1]


def search_dw(lib, cls, calls, names):
    best = None
    which = cls[1]
    if which == 'bwd_dx':
        k, s, pad, flag = cls[3], cls[4], cls[5], cls[6]
    else:
        k, s, pad, flag = cls[2], cls[3], cls[4], cls[5]
    for B in DW_B:
        for C in DW_C:
            for H in DW_H:
                if best and B * H * C > best[0][0]:
                    break
                for W in DW_W:
                    call = ('dw', which, B, H, W, C, k, s, pad, flag)
                    c = cost(call)
                    if c[0] > LIMIT[0] or (best and c >= best[0]):
                        break
                    if _ok(lib, call, cls, names):
                        best = (c, call)
                        break
    return best and best[1]


SEARCH = {'nt': search_nt, 'tn': search_tn, 'dw': search_dw}


def main():
    lib = _lib.load()
    used = tc.used_classes(lib)
    lines, over = [], []
    for cls in sorted(used, key=repr):
        LIMIT[0] = tc.MAX_ELEMS
        hit = SEARCH[cls[0]](lib, cls, used[cls], ())
        if not hit:                                            # no problem of this class is that small: the cheapest one, recorded
            LIMIT[0] = tc.OVER_LIMIT_FACTOR * tc.MAX_ELEMS
            hit = SEARCH[cls[0]](lib, cls, used[cls], ())
            over.append(cls)
        assert hit, ('no case within the element limit', cls)
        lines.append((hit, cls, ()))
        app = tc.applicable(cls)
        for combo in tc.COMBOS[cls[0]]:
            names = tuple(n for n in combo if n in app)
            if not names:
                continue
            hit = SEARCH[cls[0]](lib, cls, used[cls], names)
            if hit:
                lines.append((hit, cls, names))
                continue
            for n in names:                                    # not jointly: one case per edge
                hit = SEARCH[cls[0]](lib, cls, used[cls], (n,))
                if hit:
                    lines.append((hit, cls, (n,)))
                else:
                    print('# not reachable: %r: %s' % (cls, n))
    write_table(used, lines, over)


def write_table(used, lines, over):
    """lines: (problem, class, edge names).  One row per (problem, class): a problem found for several edge lists carries them all,
    and the cheapest problem of a class is no row of its own where it already carries edges"""
    merged = collections.OrderedDict()
    for case, cls, edges in lines:
        merged.setdefault((case, cls), set()).update(edges)
    order = {kind: [e[0] for e in tc.EDGES[kind]] for kind in tc.EDGES}
    rows = ['    %r,\n' % (case + (cls, tuple(n for n in order[case[0]] if n in names)),) for (case, cls), names in merged.items()]
    counts = collections.Counter(tc.family(c) for c in used)
    block = ('# classes per kernel that the sweep of all_swept_calls() finds (recorded in DESIGN.md; the host test recounts them)\n'
             'CLASS_COUNTS = {\n%s}\n\n# classes that no problem within MAX_ELEMS reaches (their cases are the cheapest that do)\n'
             'OVER_LIMIT = [\n%s]\n\n# fmt: off\nCASES = [\n%s]\n# fmt: on\n'
             % (''.join('    %r: %d,\n' % kv for kv in sorted(counts.items())), ''.join('    %r,\n' % (c,) for c in over), ''.join(rows)))
    path = os.path.join(ROOT, 'tests', '_train_cases.py')
    with open(path) as f:
        src = f.read()
    head, rest = src.split('# CASES-BEGIN\n')
    tail = rest.split('# CASES-END\n')[1]
    with open(path, 'w') as f:
        f.write(head + '# CASES-BEGIN\n' + block + '# CASES-END\n' + tail)
    print('%d classes, %d cases written to %s' % (len(used), len(rows), path))


def old_calls():
    """the calls that the parametrize lists (and fixed shapes) of the six older kernel-level tests of tests/test_train_gpu.py make"""
    import test_train_gpu as t

    def shapes(fn):
        return [a for m in fn.pytestmark if m.name == 'parametrize' for a in m.args[1]]
    calls = []
    for M, K, N in shapes(t.test_gemm_nt):
        calls.append(tc._nt('gemm_nt', M, K, N, tc.BIAS))
    for M, N, K in shapes(t.test_gemm_tn):
        calls.append(tc._tn('gemm_tn', M, N, K))
    for k, s, H, W, C in shapes(t.test_dwconv_backward):
        calls += [('dw', 'bwd_dx', 2, H, W, C, k, s, 0, 0), ('dw', 'bwd_dw', 2, H, W, C, k, s, 0, 0), ('dw', 'bwd_dw', 2, H, W, C, k, s, 0, 1)]
    B, hw, NO, K, P = 3, 12, 54, 64, 30                       # test_gemm_row_maps_packed_levels
    pk = (hw, P * NO, NO)
    calls += [tc._nt('gemm_nt', B * hw, K, NO, ckind=tc.STRIDED, pk=pk), tc._tn('gemm_tn', B * hw, NO, K, ykind=tc.STRIDED, pk=pk),
              tc._nt('gemm_nt', B * hw, NO, K, akind=tc.STRIDED, pk=pk)]
    for hws in shapes(t.test_levels_ops_match_per_level_torch):
        lv = (3, tuple(hws))
        M, Pp = tc.levels_rows(lv), sum(h * w for h, w in hws)
        for N in (36, 270):
            pk = (0, Pp * N, N)
            calls.append(tc._tn('gemm_tn_levels', M, N, 64, ykind=tc.LEVELS, pk=pk, lv=lv))
            if N == 36:
                calls += [tc._nt('gemm_nt_levels', M, 64, N, tc.BIAS, ckind=tc.LEVELS, pk=pk, lv=lv),
                          tc._nt('gemm_nt_levels', M, N, 64, akind=tc.LEVELS, pk=pk, lv=lv)]
    for H, W, C, k, s in shapes(t.test_fused_mbconv_kernels):
        B, N = 3, 16
        Ho, Wo = tc.same_out(H, s), tc.same_out(W, s)
        M = B * Ho * Wo
        # shift / bias are whole tensors there: 16-byte aligned
        calls += [('dw', 'fwd', B, H, W, C, k, s, 0, 1), ('dw', 'fwd', B, H, W, C, k, s, 0, 0), ('dw', 'bwd_dx', B, H, W, C, k, s, 0, 1),
                  tc._nt('gemm_nt_fused', M, C, N, tc.BIAS | tc.A_SCALE | tc.RES | tc.C2, Ho * Wo),
                  tc._nt('gemm_nt_fused', M, C, N, tc.BIAS | tc.A_SCALE | tc.RES, Ho * Wo),
                  tc._nt('gemm_nt_fused', M, C, N, tc.BIAS | tc.C2), tc._tn('gemm_tn_scaled', M, N, C, Ho * Wo)]
    return calls


def old_coverage():
    lib = _lib.load()
    used = tc.used_classes(lib)
    reached = {tc.call_class(lib, c) for c in old_calls()}
    cases = collections.Counter(tc.family(c[-2]) for c in tc.CASES)
    tot = collections.Counter(tc.family(c) for c in used)
    hit = collections.Counter(tc.family(c) for c in used if c in reached)
    print('%-34s %7s %13s %5s' % ('kernel', 'classes', 'older tests', 'cases'))
    for key in sorted(tot):
        print('%-34s %7d %13d %5d' % (key, tot[key], hit[key], cases[key]))
    print('%-34s %7d %13d %5d' % ('total', sum(tot.values()), sum(hit.values()), len(tc.CASES)))
    return tot, hit, cases


if __name__ == '__main__':
    old_coverage() if '--old-coverage' in sys.argv[1:] else main()
