"""Host checks behind tests/test_dwconv_forms_gpu.py (no GPU): the contract of effdet_dwconv_plan_describe; the geometry it reports
is the one effdet_dwconv_blocks_per_image sizes the pool-partial buffers by, on every case; the table of tests/_dwconv_cases.py
holds the geometries it names; the float64 references agree with oracle.model's float32 arithmetic, and the GPU test's bounds
separate them from references with one fault a kernel could have."""
import ctypes

import pytest
import torch

import _dwconv_cases as dc

EINVAL = -22


@pytest.fixture(scope='module')
def lib():
    from ood_object_detection_amd import _lib
    return _lib.load()


def test_plan_query_contract(lib):
    """slot order, truncation to n, the pad flag selects the pads and is otherwise stripped, what the launch refuses is refused"""
    n = dc.PLAN_INTS
    out = (ctypes.c_int * n)()
    args = (1, 34, 30, 144, 5, 2, 1)
    assert lib.effdet_dwconv_plan_describe(*args, out, n) == n
    full = list(out)
    p = dict(zip(dc.FIELDS, full))
    # 18 groups of 8 channels: 14 pixels in flight, 252 threads, 112 pixels per workgroup, 17 x 15 = 255 pixels in 3 workgroups;
    # TF-SAME pads of a 5 x 5 / s2 window on even sizes: 1; pool staging [PT][C] floats
    assert (p['KS'], p['nz'], p['CG'], p['PT'], p['threads'], p['ppb'], p['blocks'], p['pad_t'], p['pad_l'], p['lds']) == \
        (5, 1, 18, 14, 252, 112, 3, 1, 1, 14 * 144 * 4)
    for i in range(n):
        out[i] = -7
    assert lib.effdet_dwconv_plan_describe(*args, out, 4) == 4
    assert list(out)[:4] == full[:4] and all(v == -7 for v in list(out)[4:])
    assert lib.effdet_dwconv_plan_describe(*args, out, n + 3) == n
    assert lib.effdet_dwconv_plan_describe(*args, None, n) == EINVAL and lib.effdet_dwconv_plan_describe(*args, out, 0) == EINVAL
    assert lib.effdet_dwconv_plan_describe(args[0] | dc.PAD, *args[1:], out, n) == n
    sym = dict(zip(dc.FIELDS, out))
    assert (sym['pad_t'], sym['pad_l']) == (2, 2) and {k: v for k, v in sym.items() if k[:3] != 'pad'} == {k: v for k, v in p.items() if k[:3] != 'pad'}
    assert dc.plan(lib, 1, 34, 30, 144, 5, 2, pooled=False)['lds'] == 0
    q = dc.plan(lib, 2, 4, 3, 3072, 3, 1)
    assert (q['nz'], q['CG'], q['PT'], q['threads'], q['ppb'], q['blocks']) == (2, 192, 1, 192, 8, 2)
    q = dc.plan(lib, 0, 5, 7, 8, 3, 1)
    assert (q['nz'], q['CG'], q['PT'], q['threads'], q['ppb'], q['blocks']) == (1, 1, 256, 256, 256, 1)      # a map below one share
    for bad in ((3, 8, 8, 8, 3, 1), (-1, 8, 8, 8, 3, 1), (1, 0, 8, 8, 3, 1), (1, 8, 0, 8, 3, 1), (1, 8, 8, 12, 3, 1), (1, 8, 8, 0, 3, 1),
                (1, 8, 8, 8, 4, 1), (1, 8, 8, 8, 7, 1), (1, 8, 8, 8, 3, 3), (1, 8, 8, 8, 3, 0)):
        assert lib.effdet_dwconv_plan_describe(*bad, 1, out, n) == EINVAL, bad
    assert lib.effdet_dwconv_blocks_per_image(0, 4, 8) == EINVAL and lib.effdet_dwconv_blocks_per_image(4, 4, 12) == EINVAL


def test_blocks_per_image_is_the_describe_slot(lib):
    """on every depthwise case and pad convention, and over every backbone width at a few maps"""
    for case in dc.DW_CASES:
        dt, C, H, W, k, s = case
        for sym in (False, True):
            p = dc.case_plan(lib, case, sym=sym)
            assert p['blocks'] == lib.effdet_dwconv_blocks_per_image((H + s - 1) // s, (W + s - 1) // s, C), case
            assert (p['pad_t'], p['pad_l']) == (dc.pads(H, k, s, sym), dc.pads(W, k, s, sym)), case
            assert p['threads'] == p['CG'] * p['PT'] <= 256 and p['nz'] * p['CG'] * 8 == C and p['ppb'] % p['PT'] == 0
    for C in range(8, 4104, 8):
        for hw in ((1, 1), (5, 5), (20, 20), (64, 64)):
            assert dc.plan(lib, 0, hw[0], hw[1], C, 3, 1)['blocks'] == lib.effdet_dwconv_blocks_per_image(hw[0], hw[1], C)


def test_the_table_holds_the_named_geometries(lib):
    for dt in (0, 1, 2):
        for k in (3, 5):
            for s in (1, 2):
                ps = {c[1:4]: (dc.case_plan(lib, c), ((c[2] + s - 1) // s) * ((c[3] + s - 1) // s)) for c in dc.DW_CASES if (c[0], c[4], c[5]) == (dt, k, s)}
                assert any(p['nz'] == 2 for p, _ in ps.values())                                     # channel slices
                assert any(p['PT'] == 1 and p['nz'] == 1 for p, _ in ps.values())                    # one pixel in flight
                assert any(p['threads'] == 252 for p, _ in ps.values())                              # 18 groups do not divide 256
                assert any(p['CG'] == 1 and npix < 2048 for p, npix in ps.values())                  # a map below one share
                assert any(p['blocks'] > 1 and npix % p['ppb'] for p, npix in ps.values())           # a partial last workgroup
                assert any(m[1] == 1 for m in ps) and any(m[2] == 1 for m in ps)                     # H = 1, W = 1
    # the conventions differ on some case of every stride-2 kernel, in pad_t and in pad_l
    for k in (3, 5):
        assert any(dc.pads(c[2], k, 2, False) != dc.pads(c[2], k, 2, True) for c in dc.DW_CASES if c[4:] == (k, 2))
        assert any(dc.pads(c[3], k, 2, False) != dc.pads(c[3], k, 2, True) for c in dc.DW_CASES if c[4:] == (k, 2))


@pytest.mark.parametrize('case', dc.DW_CASES, ids=[dc.case_id(c) for c in dc.DW_CASES])
def test_reference_and_yardstick(lib, case):
    """R64 agrees with oracle.model's float32 arithmetic within 2e-5; the GPU test's bounds separate R64 from the other convention's
    pads and from a tap dropped at the border wherever those can change the case, and the pool sums of R64 from sums that miss a
    share's last pixel"""
    d = dc.dw_inputs(case)
    dt = case[0]
    seen = set()
    for sym in (False, True):
        p = dc.case_plan(lib, case, sym=sym)
        for act in (1, 0):
            r64 = dc.dw_ref(case, d, sym, act)
            top = float(r64.abs().max())
            assert float((dc.dw_oracle_f32(case, d, sym, act).double() - r64).abs().max()) < dc.F32_TOL * top
            bnd, e_q = dc.dw_bound(dt, r64)
            if e_q is not None:
                assert 2.0 ** -12 < e_q <= 2.0 ** -8, e_q
            for defect in dc.DEFECTS:
                bad = dc.dw_ref(case, d, sym, act, defect=defect)
                if bad is not None:
                    seen.add(defect)
                    assert float((bad - r64).abs().max()) > bnd, (sym, act, defect, float((bad - r64).abs().max()) / top, e_q)
        y = r64.reshape(dc.B, -1, case[1]) if dt != 1 else None
        y = dc.pr.bf16_round(r64).reshape(dc.B, -1, case[1]) if dt == 1 else y
        good, bad = dc.pool_blocks(y, p['ppb'], p['blocks']), dc.pool_blocks(y, p['ppb'], p['blocks'], drop_last=True)
        assert bool(((bad - good).abs() > dc.pool_bound(dt, y, p['ppb'], p['blocks'])).any())
    assert dc.DEFECTS[1] in seen


def test_se_and_maxpool_references():
    """the float64 SE gate against oracle.model._se; the max-pool reference is oracle.model.maxpool_pad itself, exact"""
    for C in dc.SE_C:
        for nblk in dc.SE_NBLK:
            for R in dc.SE_R:
                d = dc.se_inputs(C, nblk, R)
                ref = dc.se_ref(d)
                assert float((dc.se_oracle_f32(d) - ref).abs().max()) < dc.F32_TOL * float(ref.abs().max()), (C, nblk, R)
    for case in dc.POOL_CASES:
        x = dc.pool_inputs(case)
        same, sym = dc.pool_ref(x, False), dc.pool_ref(x, True)
        assert same.shape == sym.shape == (dc.B, (case[2] + 1) // 2, (case[3] + 1) // 2, case[1])
        assert bool(torch.isfinite(same).all()) and bool(torch.isfinite(sym).all())
    assert any(not torch.equal(dc.pool_ref(dc.pool_inputs(c), False), dc.pool_ref(dc.pool_inputs(c), True)) for c in dc.POOL_CASES)
