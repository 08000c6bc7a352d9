"""Host checks behind tests/test_sepconv_forms_gpu.py (no GPU): the contract of effdet_sepconv_plan_describe; the case table of
tests/_sepconv_cases.py reaches every class of the fused separable conv that the d0 ... d5 networks and AnchorNet use - asked of
the launcher's own dispatch - and still reaches the class each case is listed for; on every case the float64 reference R64 agrees
with oracle.model's float32 arithmetic, and the GPU test's bound separates R64 from references with one fault a kernel could have."""
import collections
import ctypes

import pytest
import torch

import _sepconv_cases as sc
import _sepconv_ref as sr

IDS = ['%03d-%s' % (i, sc.case_id(c)) for i, c in enumerate(sc.CASES)]
EINVAL = -22


@pytest.fixture(scope='module')
def lib():
    from ood_object_detection_amd import _lib
    return _lib.load()


def _query(lib, dtype, hw, n_in, F, N, C, A, scale, act, aligned, out, n):
    chw = (ctypes.c_int * (2 * len(hw)))(*[v for p in hw for v in p]) if hw is not None else None
    return lib.effdet_sepconv_plan_describe(dtype, len(hw) if hw is not None else 1, chw, n_in, F, N, C, A, scale, act, aligned, out, n)


def test_plan_query_contract(lib):
    """slot order, truncation to n, the pad flag is stripped, what the launch refuses is refused"""
    n = sc.PLAN_INTS
    out = (ctypes.c_int * n)()
    hw = sc.HEAD_HW
    args = (1, hw, 1, 64, 810, 90, 9, 0, 0, 1)
    assert _query(lib, *args, out, n) == n
    full = list(out)
    p = dict(zip(sc.FIELDS, full))
    tiles = sum(((h + 7) // 8) * ((w + 15) // 16) for h, w in hw)
    assert (p['kind'], p['TH'], p['TW'], p['threads'], p['FT'], p['BN']) == (1, 8, 16, 512, 64, 96)
    assert (p['OOD'], p['BST'], p['NIN'], p['META'], p['subs'], p['nchunks'], p['tiles_total']) == (1, 1, 3, 0, 1, 9, tiles)
    assert 0 < p['lds'] <= 64 * 1024 and p['taps_prefetched'] == 1 and p['w_prefetched'] == 1 and p['out_f32'] == 0 and p['vec_ok'] == 1
    for i in range(n):
        out[i] = -7
    assert _query(lib, *args, out, 5) == 5
    assert list(out)[:5] == full[:5] and all(v == -7 for v in list(out)[5:])
    assert _query(lib, args[0] | sc.PAD, *args[1:], out, n) == n and list(out) == full
    assert _query(lib, *args, out, n + 4) == n
    assert _query(lib, *args, None, n) == EINVAL and _query(lib, *args, out, 0) == EINVAL
    # unaligned outputs: vec_ok off, and with it the branch-free class predict
    assert _query(lib, *args[:-1], 0, out, n) == n
    q = dict(zip(sc.FIELDS, out))
    assert q['vec_ok'] == 0 and q['BST'] == 0 and q['BN'] == 96 and q['TH'] == 8
    # what the launch refuses: dtype, levels, n_in, F, N, anchors x classes != N, a tile beyond 160 KiB of LDS
    for bad in ((4, hw, 1, 64, 810, 90, 9, 0, 0, 1), (1, hw + [(1, 1)], 1, 64, 810, 90, 9, 0, 0, 1), (1, [(0, 4)], 1, 64, 64, 0, 9, 1, 0, 1),
                (1, hw, 4, 64, 64, 0, 9, 1, 0, 1), (1, hw, 0, 64, 64, 0, 9, 1, 0, 1), (1, hw, 1, 60, 64, 0, 9, 1, 0, 1),
                (1, hw, 1, 0, 64, 0, 9, 1, 0, 1), (1, hw, 1, 64, 0, 0, 9, 1, 0, 1), (1, hw, 1, 64, 800, 90, 9, 0, 0, 1),
                (1, hw, 1, 64, 810, 90, 0, 0, 0, 1), (0, hw, 1, 512, 512, 0, 9, 1, 0, 1), (2, hw, 1, 64, 36, 0, 9, 0, 0, 1),
                (2, hw, 1, 64, 64, 0, 9, 1, 0, 0), (1, None, 1, 64, 64, 0, 9, 1, 0, 1)):
        assert _query(lib, *bad, out, n) == EINVAL, bad
    # float32 at 288: the 96-class chunk does not fit, 64-class sub-chunks carry max and sum-exp; dtype 3 reports float32 outputs
    p = sc.plan(lib, 0, hw, 1, 288, 810, 90, False, False, True)
    assert (p['kind'], p['TW'], p['threads'], p['FT'], p['BN'], p['subs'], p['nchunks']) == (0, 8, 256, 0, 64, 2, 18) and p['lds'] > 64 * 1024
    p = sc.plan(lib, 3, hw, 1, 160, 36, 0, False, False, True)
    assert (p['kind'], p['out_f32'], p['FT'], p['BN'], p['OOD'], p['nchunks'], p['vec_ok']) == (1, 1, 160, 64, 0, 1, 1)
    # the taps switch: 9 F <= 1536 (512 threads) / 1280 (256 threads)
    assert [sc.plan(lib, dt, [sc.NODE_HW], 3, F, F, 0, True, False, True)['taps_prefetched'] for dt, F in
            ((1, 168), (1, 176), (0, 136), (0, 144))] == [1, 0, 1, 0]
    assert lib.effdet_sepconv_tiles(1, len(hw), (ctypes.c_int * 10)(*[v for q in hw for v in q]), None) == tiles


def test_every_used_class_has_a_case(lib):
    """every class of every call the networks make has a case whose own plan has that class: the share of used classes left
    out is zero; and a case still reaches the class it is in the table for"""
    used = sc.used_classes(lib)
    have = collections.Counter()
    for case in sc.CASES:
        got = sc.klass(sc.case_plan(lib, case))
        assert got == case[6], ('the case no longer reaches the class it is in the table for', case, got)
        have[got] += 1
    for c in sorted(used):
        print(c, '%d cases, e.g. used by %s %s' % (have[c], used[c][0], used[c][1]))
    print('total %d used classes, %d classes in the table, %d cases' % (len(used), len(have), len(sc.CASES)))
    missing = sorted(c for c in used if not have[c])
    assert not missing, ['%r, e.g. %r' % (c, used[c]) for c in missing]
    assert len(set(c[:6] for c in sc.CASES)) == len(sc.CASES)


def test_the_table_holds_the_named_cases(lib):
    """per dtype and width: every node kind, a head layer, the box predict (dtype 3 for bf16), AnchorNet's layers and predict, the
    class counts that cut the chunks; per bf16 class-predict form a case with vec_ok off by an odd stride and one with it on; and every form with
    subs > 1 has a case whose last sub-chunk holds one class and one whose sub-chunks are all full"""
    keys = {c[:6] for c in sc.CASES}
    for dt in (0, 1):
        for F in sc.WIDTHS:
            assert all(('node', dt, F, F, 0, k) in keys for k in sc.NODE_KINDS)
            assert ('layer', dt, F, F, 0, '') in keys and ('layer', dt, F, sc.ANCHOR_CH, 0, '') in keys
            assert ('box', 3 if dt else 0, F, 36, 0, '') in keys
            want = {64: (1, 2, 7, 90, 96, 98, 150), 88: (1, 2, 7, 90, 96, 98, 150), 288: (1, 64, 65, 90, 128)}.get(F, (7, 90))
            assert all(('cls', dt, F, 9 * C, C, 'aligned') in keys for C in want + (400,))
        assert ('anchor', dt, sc.ANCHOR_CH, 9, 0, '') in keys
    # every bf16 class-predict form but the branch-free one (which cannot run without vec_ok) has a case whose even row length
    # leaves vec_ok to the image stride and whose odd stride turns it off, and a case with vec_ok on (at 64 channels a single
    # aligned chunk of an even class count is the branch-free form, so the general one-chunk form there never sees vec_ok on)
    forms = collections.defaultdict(set)
    for c in sc.CASES:
        if c[0] == 'cls' and c[1] == 1:
            forms[c[6]].add((c[5], c[4] % 2, sc.case_plan(lib, c)['vec_ok']))
    assert len(forms) == 13 and sum(1 for k in forms if k[7]) == 1
    for k, seen in forms.items():
        if k[7]:                                                      # BST
            assert {v for _, _, v in seen} == {1}, k
            continue
        assert ('odd', 0, 0) in seen, k
        assert ('aligned', 0, 1) in seen or (k[4] == 64 and not k[9]), k
    tails = collections.defaultdict(set)
    for c in sc.CASES:
        p = sc.case_plan(lib, c)
        if p['subs'] > 1:
            tails[c[6]].add(c[4] % p['BN'])
    assert tails and all({0, 1} <= t for t in tails.values()), dict(tails)
    d = sc.make_inputs(('node', 1, 64, 64, 0, '3in-fast'))
    assert float(d['ins'][0][2][0].max()) < 0 and d['ins'][0][2][0].shape[-2:] == (36, 67)     # the pooled input is all negative


def _applicable(case, p):
    out = [sr.DEFECTS[0], sr.DEFECTS[1], sr.DEFECTS[3]]
    if case[0] == 'node':
        pool = sc.NODE_KINDS[case[5]][1]
        if pool and sr.pool_pads(sc.POOL_HW[pool][1], False) != sr.pool_pads(sc.POOL_HW[pool][1], True):
            out.append(sr.DEFECTS[2])                                 # (an odd width pads 1 on the left in both conventions)
    return out


def test_the_pad_defect_has_cases():
    assert sum(1 for c in sc.CASES if sr.DEFECTS[2] in _applicable(c, None)) == 24      # two node kinds x six widths x two dtypes


@pytest.mark.parametrize('case', sc.CASES, ids=IDS)
def test_reference_and_yardstick(lib, case):
    """on the GPU test's own inputs, per max-pool convention: R64 agrees with oracle.model's float32 arithmetic within the
    project's 2e-5; the GPU test's bound (float32 2e-5, bf16 2 e_q with e_q = the rounded reference's own error) separates R64
    from every defective reference that applies - judged on the first bias pattern - and, where an anchor's classes run as
    sub-chunks, its energy bound separates the float64 energy from a carry that forgets to rescale the running sum-exp when a
    later sub-chunk raises the max (bias pattern 'max first / last')"""
    d = sc.make_inputs(case)
    p = sc.case_plan(lib, case)
    dtype, N, C = case[1], case[3], case[4]
    for pad in d['pads']:
        r64 = sc.reference(case, d, pad)
        rq = sc.reference(case, d, pad, quant=True) if dtype != 0 else [None] * len(r64)
        bnd, e_q = sc.bound(case, r64[0], rq[0])
        # R64 against the oracle's float32 arithmetic
        lv = [sr.oracle_f32([x for x, _ in ins], [m for _, m in ins], d['fw'], d['den'], d['fuse_mode'], d['pre_act'], d['dw'], d['pw'],
                            None if d['scale'] is None else d['scale'][r], d['shifts'][0][1][r], d['post_act'], pad)
              for ins, r in zip(d['ins'], d['affine_rows'])]
        o32 = torch.cat([y.permute(0, 2, 3, 1).reshape(sc.B, -1, N) for y in lv], 1)
        assert sc.rel_err(o32, r64[0]) < sc.F32_TOL, (pad, sc.rel_err(o32, r64[0]))
        if dtype != 0:
            assert 2.0 ** -11 < e_q < 2.0 ** -6, (pad, e_q)                       # a bf16 kernel's error: some roundings, not more
        for defect in _applicable(case, p):
            bad = sc.reference(case, d, pad, defect=defect)[0]
            err = sc.rel_err(bad, r64[0])
            assert err > bnd, (pad, defect, err, bnd)
        if p['subs'] > 1:
            z = r64[1].reshape(sc.B, -1, sc.A, C)
            e_ref, _ = sr.ood_ref(z)
            assert float((sr.energy_carry(z, p['BN']) - e_ref).abs().max()) < 1e-9
            b1 = sc.bound(case, r64[1], rq[1])[0]
            err = float((sr.energy_carry(z, p['BN'], rescale=False) - e_ref).abs().max())
            assert err > sc.score_bound(b1, r64[1], e_ref), (err, sc.score_bound(b1, r64[1], e_ref))
