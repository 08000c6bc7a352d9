"""Host checks behind tests/test_pw_gemm_forms_gpu.py (no GPU): the contract of effdet_pw_gemm_plan_describe and
effdet_pw_gemm_group_plan_describe; the case table of tests/_pw_gemm_cases.py reaches every class of the 1x1-conv GEMM that the
d0 ... d5 networks of both families (own image size, batch 1 and 16), MetaHead and ProjectionNet use - asked of the launchers'
own dispatch - and still reaches the class each case was made for; on every case the float64 reference R64 agrees with
oracle.model's float32 arithmetic, and the GPU test's bound separates R64 from references with one fault a kernel could have."""
import collections
import ctypes

import pytest
import torch

import _pw_gemm_cases as pc
import _pw_gemm_ref as pr

IDS = ['%03d-%s' % (i, pc.case_id(c)) for i, c in enumerate(pc.CASES)]
EINVAL = -22


@pytest.fixture(scope='module')
def lib():
    from ood_object_detection_amd import _lib
    return _lib.load()


def _q(lib, dtype, M, K, N, rpi, gated, res, ldc, cis, aligned, group, out, n):
    return lib.effdet_pw_gemm_plan_describe(dtype, M, K, N, rpi, gated, res, ldc, cis, aligned, group, out, n)


def test_plan_query_contract(lib):
    """slot order, truncation to n, the pad flag is stripped, what the launch refuses is refused"""
    n = pc.PLAN_INTS
    out = (ctypes.c_int * n)()
    # a d0 project conv at batch 16: 16 images of 64 x 64 pixels, mid 96 -> 24 channels, gate + residual, bf16
    args = (1, 16 * 4096, 96, 24, 4096, 1, 1, 0, 0, 1, 0)
    assert _q(lib, *args, out, n) == n
    full = list(out)
    p = dict(zip(pc.FIELDS, full))
    assert (p['BN'], p['PT'], p['NTH'], p['GATED'], p['tiles_per_image'], p['n_tiles'], p['blocks'], p['small']) == (32, 2, 256, 1, 32, 1, 512, 0)
    assert (p['vec_ok'], p['kchunks'], p['nst'], p['KPC']) == (1, 3, 2, 32)
    assert p['lds'] == 2 * 32 * (2 * 64 + 16) + 96 * 4                 # two weight images of BN rows of one stage + 16 bytes, the gate
    for i in range(n):
        out[i] = -7
    assert _q(lib, *args, out, 5) == 5
    assert list(out)[:5] == full[:5] and all(v == -7 for v in list(out)[5:])
    assert _q(lib, args[0] | pc.PAD, *args[1:], out, n) == n and list(out) == full
    assert _q(lib, *args, out, n + 4) == n
    assert _q(lib, *args, None, n) == EINVAL and _q(lib, *args, out, 0) == EINVAL
    # one image less: 480 workgroups, the small form; the 128 tile keeps 256 threads and reports itself, never 96
    q = pc.plan(lib, 1, 15 * 4096, 96, 24, 4096, True, True)
    assert (q['BN'], q['PT'], q['NTH'], q['small'], q['blocks']) == (32, 1, 512, 1, 480)
    q = pc.plan(lib, 1, 300, 96, 128, 0)
    assert (q['BN'], q['PT'], q['NTH'], q['small'], q['GATED']) == (128, 2, 256, 1, 0)
    # the tile: the smallest of 32 ... 192 that covers N, else equal tiles
    assert [pc.plan(lib, 0, 64, 8, N)['BN'] for N in (8, 32, 33, 96, 104, 136, 192, 200, 384, 392, 810)] == \
        [32, 32, 64, 96, 128, 160, 192, 128, 192, 160, 192]
    assert [pc.plan(lib, 0, 64, 8, N)['n_tiles'] for N in (192, 200, 384, 392, 810)] == [1, 2, 2, 3, 5]
    # vec_ok: whole 16-byte rows, row pitch and image stride, aligned pointers
    v = lambda dt, N, ldc, cis, al=1: pc.plan(lib, dt, 100, 16, N, 50, False, True, ldc, cis, al)['vec_ok']
    assert [v(1, 24, 0, 0), v(1, 9, 0, 0), v(1, 24, 32, 1616), v(1, 24, 32, 1618), v(1, 24, 28, 0), v(1, 24, 0, 0, 0)] == [1, 0, 1, 0, 0, 0]
    assert [v(0, 24, 0, 0), v(0, 9, 0, 0), v(0, 24, 32, 1616), v(0, 24, 32, 1618), v(0, 810, 0, 0)] == [1, 0, 1, 0, 0]
    # K-chunks and stages per dtype
    assert [(pc.plan(lib, dt, 64, K, 8)['kchunks'], pc.plan(lib, dt, 64, K, 8)['nst']) for dt, K in
            ((0, 8), (0, 40), (0, 1152), (1, 40), (1, 1152), (2, 40), (2, 3072))] == [(1, 1), (3, 2), (72, 36), (2, 1), (36, 18), (2, 2), (96, 96)]
    # what the launch refuses: K % 8, M % rows_per_image, dtype, empty shapes; two-term: N % 8, ldc % 8, image stride % 8, alignment
    ok = (1, 100, 16, 24, 50, 0, 0, 0, 0, 1, 0)
    assert _q(lib, *ok, out, n) == n
    for bad in ((1, 100, 12, 24, 50, 0, 0, 0, 0, 1, 0), (1, 100, 16, 24, 30, 0, 0, 0, 0, 1, 0), (3, 100, 16, 24, 50, 0, 0, 0, 0, 1, 0),
                (-1, 100, 16, 24, 50, 0, 0, 0, 0, 1, 0), (1, 0, 16, 24, 0, 0, 0, 0, 0, 1, 0), (1, 100, 0, 24, 50, 0, 0, 0, 0, 1, 0),
                (1, 100, 16, 0, 50, 0, 0, 0, 0, 1, 0), (1, 1 << 31, 16, 24, 0, 0, 0, 0, 0, 1, 0),
                (2, 100, 16, 9, 50, 0, 0, 0, 0, 1, 0), (2, 100, 16, 24, 50, 0, 0, 28, 0, 1, 0), (2, 100, 16, 24, 50, 0, 0, 32, 1604, 1, 0),
                (2, 100, 16, 24, 50, 0, 0, 0, 0, 0, 0),
                # as a group: a gate, a residual, a strided output, images, a tile beyond 96
                (1, 100, 16, 24, 0, 1, 0, 0, 0, 1, 1), (1, 100, 16, 24, 0, 0, 1, 0, 0, 1, 1), (1, 100, 16, 24, 0, 0, 0, 32, 0, 1, 1),
                (1, 100, 16, 24, 50, 0, 0, 0, 0, 1, 1), (1, 100, 16, 104, 0, 0, 0, 0, 0, 1, 1), (2, 100, 16, 12, 0, 0, 0, 0, 0, 1, 1)):
        assert _q(lib, *bad, out, n) == EINVAL, bad
    assert _q(lib, 1, 100, 16, 96, 0, 0, 0, 0, 0, 1, 1, out, n) == n and list(out)[:3] == [96, 1, 512]


def test_act_is_checked_by_the_shared_path(lib):
    """act outside 0 ... 2 is refused by the function the describe query runs too: the launch returns before it touches a pointer
    or the device (null stream, stand-in pointers that are never read)"""
    for act in (-1, 3):
        assert lib.effdet_pw_gemm_bn_act(None, 1, 64, 100, 16, 64, 24, None, 64, act, None, None, 50, 64, 0, 0) == EINVAL
    one = lambda ct, v: (ct * 1)(v)
    assert lib.effdet_pw_gemm_group(None, 1, 1, one(ctypes.c_void_p, 64), one(ctypes.c_longlong, 100), one(ctypes.c_int, 16),
                                    one(ctypes.c_void_p, 64), one(ctypes.c_int, 24), one(ctypes.c_void_p, 64), one(ctypes.c_void_p, 64),
                                    3, one(ctypes.c_void_p, 64)) == EINVAL


def test_group_query_contract(lib):
    """the group launcher's rules: one tile shape, BN <= 96, at most 8 problems; the launch total decides the form; per-problem slots"""
    n = pc.PLAN_INTS
    probs = [(40002, 40, 88), (5, 72, 88), (26000, 16, 88)]
    p0, p1 = pc.group_plan(lib, 1, probs, 0), pc.group_plan(lib, 1, probs, 1)
    assert (p0['BN'], p0['PT'], p0['NTH'], p0['GATED'], p0['small'], p0['blocks']) == (96, 2, 256, 0, 0, 313 + 1 + 204)
    assert (p0['tiles_per_image'], p0['kchunks'], p0['nst']) == (313, 2, 1) and (p1['tiles_per_image'], p1['kchunks'], p1['nst']) == (1, 3, 2)
    small = pc.group_plan(lib, 1, [(130, 40, 64), (5, 72, 64)])
    assert (small['BN'], small['PT'], small['NTH'], small['small'], small['blocks']) == (64, 1, 512, 1, 3)
    assert pc.group_plan(lib, 1, [(130, 40, 64), (5, 72, 88)]) is None                       # mixed tiles
    assert pc.group_plan(lib, 1, [(130, 40, 104)]) is None                                   # a tile beyond 96
    assert pc.group_plan(lib, 1, [(130, 40, 64)] * 8) is not None and pc.group_plan(lib, 1, [(130, 40, 64)] * 9) is None
    assert pc.group_plan(lib, 1, [(130, 44, 64)]) is None and pc.group_plan(lib, 2, [(130, 40, 60)]) is None
    assert pc.group_plan(lib, 2, [(130, 40, 64)], aligned=False) is None and pc.group_plan(lib, 1, [(130, 40, 64)], which=1) is None
    out = (ctypes.c_int * n)()
    one = lambda ct, v: (ct * 1)(v)
    assert lib.effdet_pw_gemm_group_plan_describe(1, 1, one(ctypes.c_longlong, 130), one(ctypes.c_int, 40), one(ctypes.c_int, 64), 1, 0, out, 3) == 3
    assert list(out)[:3] == [64, 1, 512]
    assert lib.effdet_pw_gemm_group_plan_describe(1, 1, one(ctypes.c_longlong, 130), one(ctypes.c_int, 40), one(ctypes.c_int, 64), 1, 0, None, 3) == EINVAL


def test_every_used_class_has_a_case(lib):
    """every class of every call the networks make has a case whose own plan has that class: the share of used classes left
    out is zero; every generated case still reaches a used class; no tensor of a case exceeds 64 MiB"""
    used = pc.used_classes(lib)
    have = collections.Counter()
    for case in pc.CASES:
        got = pc.case_classes(lib, case)
        if got is None:
            continue                                                  # refusals: test_the_table_holds_the_named_cases
        for c in set(got):
            have[c] += 1
        if case[0].startswith('form'):
            assert set(got) & set(used), ('the case no longer reaches a class the networks use', case, got)
    for c in sorted(used, key=repr):
        print(c, '%d cases, e.g. used by %s at batch %d' % (have[c], used[c][0], used[c][1]))
    print('total %d used classes, %d classes in the table, %d cases' % (len(used), len(have), len(pc.CASES)))
    missing = sorted((c for c in used if not have[c]), key=repr)
    assert not missing, ['%r, e.g. %r' % (c, used[c]) for c in missing]
    assert len(set(pc.CASES)) == len(pc.CASES)
    # both work splits of every tile but 128, gated with a residual, in every dtype; the group kernel in both forms; ReLU; MetaHead
    for dt in (0, 1, 2):
        for bn in (32, 64, 96, 160, 192):
            for pt in (1, 2):
                assert any(c[:5] == (dt, bn, pt, 1, 1) for c in have), (dt, bn, pt)
        assert any(c[:5] == (dt, 128, 2, 1, 1) for c in have)
        assert {c[2] for c in have if c[0] == dt and c[7] == 1} == {1, 2}
    for dt in (0, 1):
        assert any(c[0] == dt and c[5] == 2 for c in have) and any(c[0] == dt and c[6] == 0 and c[2] == 2 for c in have)
    for case in pc.CASES:
        es = 2 if case[1] == 1 else 4
        probs = [(p[0], p[1], p[2]) for p in case[2]] if len(case) == 4 else [(case[2] * case[3], case[4], case[5])]
        assert all(max(M * K, N * K, M * (N + 16) + 64) * es <= 64 << 20 for M, K, N in probs), case


def test_the_table_holds_the_named_cases(lib):
    """what the two-term dtype refuses is refused (N % 8, an image stride that breaks alignment) and everything else is accepted;
    'odd' turns vec_ok off and 'pitch' keeps it; the single-partial-tile problem and the scale-free problem sit in both groups"""
    named = {(c[0], c[1]): c for c in pc.NAMED}
    for (name, dt), case in named.items():
        p = pc.case_plan(lib, case)
        if dt == 2 and name in ('n9', 'n810', 'odd24', 'odd40', 'odd9'):
            assert p is None, case
            continue
        assert p is not None, case
        if name.startswith('odd'):
            assert p['vec_ok'] == 0 and case[6:8] == (name != 'odd9', True)
        if name.startswith('pitch'):
            assert p['vec_ok'] == 1 and p['GATED'] == 1 and case[7]
        if name in ('n9', 'n810'):
            assert p['vec_ok'] == 0
        if name == 'group-small':
            assert p[0]['small'] == 1 and p[1]['tiles_per_image'] == 1 and not case[2][2][3]
        if name == 'group-large':
            assert p[0]['small'] == 0 and p[0]['PT'] == 2 and p[1]['tiles_per_image'] == 1 and not case[2][2][3]
    for dt in (0, 1, 2):
        assert all(('rows%d' % r, dt) in named for r in (1, 15, 16, 17, 127, 128, 129))
        assert all(('n%d' % N, dt) in named for N in (8, 9, 16, 24, 40, 88, 810))
        assert all(('edge%d' % N, dt) in named for N in (96, 104, 128, 136, 192, 200, 384, 392))
        assert all(('noscale-act%d' % a, dt) in named for a in (0, 1, 2))
    # per dtype, one large-form case with at least four stages
    for dt in (0, 1, 2):
        assert any(c[0] == dt and c[2] == 2 and c[1] != 128 and c[8].startswith('4+')
                   for case in pc.CASES for c in (pc.case_classes(lib, case) or [])), dt


@pytest.mark.parametrize('case', pc.CASES, ids=IDS)
def test_reference_and_yardstick(lib, case):
    """on the GPU test's own inputs: R64 agrees with oracle.model's float32 arithmetic within the project's 2e-5, and the GPU
    test's bound (float32 2e-5, two-term 4e-5, bf16 2 e_q plus the gate term) separates R64 from every defective reference that
    applies: somewhere a defective element lies beyond the bound"""
    plans = pc.case_plan(lib, case)
    if plans is None:                                                 # refused by the launch: test_the_table_holds_the_named_cases
        return
    ds = pc.make_inputs(case)
    if len(case) != 4:
        plans, ds = [plans], [ds]
    for p, d in zip(plans, ds):
        r64 = pr.ref(d, p)
        top = float(r64.abs().max())
        o32 = pr.oracle_f32(d)
        assert float((o32.double() - r64).abs().max()) < pc.F32_TOL * top
        bnd, e_q = pc.bound(case[1], d, r64)
        if e_q is not None:
            assert 2.0 ** -12 < e_q <= 2.0 ** -8, e_q                  # one bf16 rounding of the output (8 significand bits)
        for defect in pr.DEFECTS:
            if not pr.applicable(defect, d, p):
                continue
            bad = pr.ref(d, p, defect=defect)
            over = ((bad - r64).abs() - bnd).max()
            assert float(over) > 0, (defect, float((bad - r64).abs().max()) / top, e_q)
