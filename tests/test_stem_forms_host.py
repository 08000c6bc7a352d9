"""Host checks behind tests/test_stem_forms_gpu.py (no GPU): the contract of effdet_stem_dw_plan_describe; the table of
tests/_stem_cases.py holds the geometries it names and reaches every kernel instantiation; the query refuses what the launch
refuses; the float64 references agree with oracle.model; a float64 emulation of each form's roundings stays inside the GPU test's
bound while references with one fault a kernel could have leave it.

Measured over every case and pad convention (max over the elements of |x - R64| / bound, then the worst case): the emulations
reach 0.79 of the bf16 bound (tile form, bf16 image), 0.18 of the two-term and 0.006 of the float32 bound; the least output defect
stands at 8.8 times the bf16 bound, 2.8e3 times the two-term and 6.8e3 times the float32 bound; a pool row that misses its last
pixel at 1.8 (bf16, rolling form), 207 (two-term) and 1.1e3 (float32) times its pool bound.  The conditions asserted on every case
are emulation < 1 and defect > 1."""
import ctypes

import pytest

import _stem_cases as sc
from oracle import model as om


@pytest.fixture(scope='module')
def lib():
    from ood_object_detection_amd import _lib
    return _lib.load()


def _sd_lds(C, size):
    """sd_lds_bytes<T>(C) of csrc/stem_dw.hip: input patch [3][37][38] + 8, weights [cpad][32 T + 16 B], E [324][C + 16 B],
    reduction scratch, 13 per-channel vectors"""
    up = lambda n: (n + 15) // 16 * 16
    return up((3 * 37 * 38 + 8) * size) + up(C) * (32 * size + 16) + up(324 * (C + 16 // size) * size) + 256 * 9 * 4 + 13 * C * 4


def _sr_lds(pair):
    """pick_stem_roll: 4 waves x (4 staged rows of 72 pixels x 8 B per image plane + 2 channel tiles x 3 rows x 32 px x 16 ch + 4 pad pixels)"""
    return 4 * ((2 if pair else 1) * 4 * 576 + 2 * 3 * 32 * (64 if pair else 32) + 4 * (64 if pair else 32))


def test_plan_query_contract(lib):
    """slot order, truncation to n, the pad flag selects the pads and is otherwise stripped"""
    n = sc.PLAN_INTS
    out = (ctypes.c_int * n)()
    q = lib.effdet_stem_dw_plan_describe
    args = (1, 0, 122, 124, 32)
    assert q(*args, out, n) == n
    full = list(out)
    # roll, 9 parts, TF-SAME pads of even sizes 0, 61 x 62 outputs, 3 strips of 21, 3 bands of 21, 3 workgroups of 4 waves, not the tile form's vec_in
    assert full == [1, 9, 0, 0, 61, 62, 3, 3, 21, 21, 3, _sr_lds(False), 0]
    for i in range(n):
        out[i] = -7
    assert q(*args, out, 5) == 5
    assert list(out)[:5] == full[:5] and all(v == -7 for v in list(out)[5:])
    assert q(*args, out, n + 3) == n
    assert q(*args, None, n) == sc.EINVAL and q(*args, out, 0) == sc.EINVAL
    # the pad flag: pad_t = pad_l = 1, an odd left pad has no rolling form
    assert q(1 | sc.PAD, 0, 122, 124, 32, out, n) == n
    assert list(out) == [0, 16, 1, 1, 61, 62, 4, 4, 16, 16, 0, _sd_lds(32, 2), 0]
    assert sc.plan(lib, 1, 1, 40, 36, 40) == dict(zip(sc.FIELDS, [0, 4, 0, 0, 20, 18, 2, 2, 16, 16, 0, _sd_lds(40, 2), 1]))
    assert sc.plan(lib, 0, 2, 33, 35, 64) == dict(zip(sc.FIELDS, [0, 4, 1, 1, 17, 18, 2, 2, 16, 16, 0, _sd_lds(64, 4), 0]))
    assert sc.plan(lib, 2, 2, 16, 32, 32) == dict(zip(sc.FIELDS, [1, 1, 0, 0, 8, 16, 1, 1, 16, 8, 1, _sr_lds(True), 0]))


def test_plan_on_every_case(lib):
    """pads, output sizes, parts = effdet_stem_dw_parts, LDS bytes and the vec_in slot on every case under both conventions"""
    for case in sc.ALL_FUSED:
        dt, it, C, H, W, B = case
        for sym in (False, True):
            p = sc.case_plan(lib, case, sym)
            if p is None:
                continue
            flag = sc.PAD if sym else 0
            assert p['parts'] == lib.effdet_stem_dw_parts(dt | flag, H, W, C) == p['nx'] * p['ny'], (case, sym)
            want = (1, 1) if sym else (om.same_pad_amounts(H, 3, 2)[0], om.same_pad_amounts(W, 3, 2)[0])
            assert (p['pad_t'], p['pad_l']) == want == (sc.pads(H, sym), sc.pads(W, sym)), (case, sym)
            assert (p['Ho'], p['Wo']) == ((H + 1) // 2, (W + 1) // 2)
            assert p['nx'] == -(-p['Wo'] // p['bw']) and p['ny'] == -(-p['Ho'] // p['bh'])
            if p['roll']:
                assert dt in (1, 2) and C == 32 and p['pad_l'] % 2 == 0 and p['Wo'] >= 16 and p['Ho'] >= 8 and p['bw'] <= 30
                assert p['per_image'] == -(-p['parts'] // 4) and p['lds'] == _sr_lds(dt == 2) and p['vec_in'] == 0
            else:
                assert dt in (0, 1) and (p['bw'], p['bh'], p['per_image']) == (16, 16, 0) and p['lds'] == _sd_lds(C, 4 if dt == 0 else 2)
                assert p['vec_in'] == int(dt == 1 and it == 1 and W % 2 == 0 and p['pad_l'] % 2 == 0)


def test_the_table_holds_the_named_geometries(lib):
    """the map table of _stem_cases' docstring, for bf16 and the two-term dtype at C = 32 under TF-SAME"""
    roll = {  # (H, W): (nstrips, TWo, nbands, band_rows, per_image, pad_t)
        (16, 32): (1, 16, 1, 8, 1, 0), (15, 60): (1, 30, 1, 8, 1, 1), (17, 34): (1, 17, 1, 9, 1, 1), (82, 62): (2, 16, 2, 21, 1, 0),
        (42, 182): (4, 23, 1, 21, 1, 0), (122, 124): (3, 21, 3, 21, 3, 0)}
    assert set(roll) == set(sc.ROLL_MAPS)
    for dt, it in ((1, 0), (1, 1), (1, 2), (2, 0), (2, 2)):
        for (H, W), want in roll.items():
            p = sc.plan(lib, dt, it, H, W, 32)
            assert (p['roll'], p['nx'], p['bw'], p['ny'], p['bh'], p['per_image'], p['pad_t'], p['pad_l']) == (1,) + want + (0,), (dt, it, H, W)
    p = sc.plan(lib, 1, 0, 82, 62, 32)
    assert (p['Wo'] - p['bw'], p['Ho'] - p['bh']) == (15, 20)                       # strips of 16 and 15 columns, bands of 21 and 20 rows
    p = sc.plan(lib, 1, 0, 42, 182, 32)
    assert p['Wo'] - 3 * p['bw'] == 22
    p = sc.plan(lib, 1, 0, 122, 124, 32)
    assert (p['Ho'] - 2 * p['bh'], p['Wo'] - 2 * p['bw'], 4 * p['per_image'] - p['parts']) == (19, 20, 3)
    for it in (0, 1, 2):
        for H, W in sc.TILE_MAPS:
            assert sc.plan(lib, 0, it, H, W, 32)['roll'] == 0, (H, W)
            p = sc.plan(lib, 1, it, H, W, 32)                                         # 40x36 is a tile map in float32 and at C != 32 only
            assert p['roll'] == int((H, W) == (40, 36)) and (p['roll'] == 0 or (p['nx'], p['bw'], p['ny'], p['bh']) == (1, 18, 1, 20)), (H, W)
    for (H, W), want in {(14, 32): (7, 16, 1, 1), (16, 30): (8, 15, 1, 1), (33, 35): (17, 18, 2, 2), (5, 5): (3, 3, 1, 1), (1, 9): (1, 5, 1, 1),
                         (9, 1): (5, 1, 1, 1), (40, 36): (20, 18, 2, 2)}.items():
        p = sc.plan(lib, 1, 1, H, W, 40 if (H, W) == (40, 36) else 32)
        assert (p['Ho'], p['Wo'], p['nx'], p['ny']) == want, (H, W)
    p = sc.plan(lib, 1, 0, 33, 35, 32)
    assert (p['pad_t'], p['pad_l']) == (1, 1)
    assert sc.plan(lib, 1, 1, 40, 36, 40)['vec_in'] == 1 and sc.plan(lib, 0, 1, 40, 36, 40)['vec_in'] == 0 and sc.plan(lib, 1, 1, 33, 35, 40)['vec_in'] == 0
    # float32 never takes the rolling form; the symmetric convention never does
    for H, W in sc.ROLL_MAPS:
        assert sc.plan(lib, 0, 0, H, W, 32)['roll'] == 0 and sc.plan(lib, 1, 1, H, W, 32, sym=True)['roll'] == 0


def test_the_table_reaches_every_form(lib):
    plans = [(c, sym, sc.case_plan(lib, c, sym)) for c in sc.FUSED_CASES for sym in (False, True)]
    plans = [(c, sym, p) for c, sym, p in plans if p is not None]
    tile = {(c[0], c[1]) for c, sym, p in plans if not p['roll']}
    roll = {(c[0], c[1]) for c, sym, p in plans if p['roll']}
    assert tile == {(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2)}                  # stem_dw_kernel<float | bf16_t, 0 | 1 | 2>
    assert roll == {(1, 0), (1, 1), (1, 2), (2, 0), (2, 2)}                          # stem_roll_kernel<0 | 1 | 2, 2, bf16_t>, <0 | 2, 2, bf16p_t>
    assert {(c[0], c[1]) for c in sc.UNFUSED_CASES} == {(o, i) for o in (0, 1, 2) for i in (0, 1, 2)} - {(2, 1)}
    for sym in (False, True):                                                        # both conventions reach every tile kernel
        assert {(c[0], c[1]) for c, s, p in plans if s == sym and not p['roll']} == tile
    tp = [(c, p) for c, sym, p in plans if not p['roll']]
    rp = [(c, p) for c, sym, p in plans if p['roll']]
    assert {p['vec_in'] for c, p in tp if (c[0], c[1]) == (1, 1)} == {0, 1}
    for dt in (0, 1):
        assert any(p['lds'] > 65536 for c, p in tp if c[0] == dt) and any(p['lds'] <= 65536 for c, p in tp if c[0] == dt)
    assert {c[2] for c, p in tp} == {8, 24, 32, 40, 48, 56, 64}
    assert any(p['Ho'] < 16 and p['Wo'] < 16 for c, p in tp) and any(c[3] == 1 for c, p in tp) and any(c[4] == 1 for c, p in tp)
    assert any(p['Wo'] % 16 and (p['Wo'] % 16) % 4 for c, p in tp if p['nx'] > 1)    # Wo % 4 != 0 inside the last tile column
    for dt in (1, 2):
        mine = [(c, p) for c, p in rp if c[0] == dt]
        rows = set()
        for c, p in mine:
            rows |= {p['bh'] % 3, (p['Ho'] - (p['ny'] - 1) * p['bh']) % 3}
        assert rows == {0, 1, 2}                                                      # the row loop's three exits
        assert any(p['nx'] > 1 and p['Wo'] % p['bw'] for c, p in mine)                # a short last strip
        assert any(p['ny'] > 1 and p['Ho'] % p['bh'] for c, p in mine)                # a short last band
        assert any(p['parts'] % 4 for c, p in mine) and any(p['per_image'] > 1 and p['parts'] % 4 for c, p in mine)      # idle waves
        assert any(p['parts'] == 1 and (p['Ho'], p['Wo']) == (8, 16) for c, p in mine)
        assert any(p['nx'] > 2 for c, p in mine)
        assert {c[5] for c, p in mine} == {1, 2, 10}                                  # a second round of 8 images with returning workgroups
    # unfused: threads of the last workgroup beyond the work, and a launch below one workgroup
    work = [2 * ((c[3] + 1) // 2) * ((c[4] + 1) // 2) * c[2] // 8 for c in sc.UNFUSED_CASES]
    assert any(w % 256 and w > 256 for w in work) and any(w < 256 for w in work)


def test_the_query_refuses_what_the_launch_refuses(lib):
    for case in sc.ALL_FUSED:
        for sym in (False, True):
            assert (sc.case_plan(lib, case, sym) is None) == sc.refused(case, sym), (case, sym)
    gone = [c for c in sc.ALL_FUSED if c not in sc.FUSED_CASES]
    assert gone and all(c[0] == 2 for c in gone) and {(c[0], c[1]) for c in sc.FUSED_CASES} == set(sc.DT_PAIRS) - {(2, 1)}
    # every two-term case left is a rolling map at C = 32 (40x36 is one there)
    assert {c[2:5] for c in sc.FUSED_CASES if c[0] == 2} == {(32, h, w) for h, w in sc.ROLL_MAPS + ((40, 36),)}
    out = (ctypes.c_int * sc.PLAN_INTS)()
    for dt, it, C, H, W, sym, off, why in sc.REFUSALS:
        if off == 0:
            assert lib.effdet_stem_dw_plan_describe(dt | (sc.PAD if sym else 0), it, H, W, C, out, sc.PLAN_INTS) == sc.EINVAL, why
    for bad in ((3, 0, 16, 32, 32), (-1, 0, 16, 32, 32), (1, 3, 16, 32, 32), (1, -1, 16, 32, 32), (1, 0, 0, 32, 32), (1, 0, 16, 0, 32),
                (1, 0, 16, 32, 0), (1, 0, 16, 32, 4), (0, 0, 16, 32, 68), (0, 0, 16, 32, 72), (2, 0, 16, 32, 64), (2, 0, 16, 32, 16)):
        assert lib.effdet_stem_dw_plan_describe(*bad, out, sc.PLAN_INTS) == sc.EINVAL, bad
    for C in (8, 16, 24, 32, 40, 48, 56, 64):                                        # ... and nothing else of the widths the entry takes
        for dt in (0, 1):
            assert sc.plan(lib, dt, 2, 16, 32, C) is not None


def _ratio(a, b, bound):
    return float(((a - b).abs() / bound).max())


def fused_ratios(lib, case):
    """per pad convention the entry accepts: (emulation / bound, {defect: ratio}) with the checks of the docstring asserted"""
    dt, it, C, H, W, B = case
    d = sc.fused_inputs(case)
    out = []
    for sym in (False, True):
        p = sc.case_plan(lib, case, sym)
        if p is None:
            continue
        r = sc.ref(d, sym)
        top = float(r['y'].abs().max())
        assert float((sc.oracle_f32(d, sym).double() - r['y']).abs().max()) < sc.F32_TOL * top
        o64 = sc.oracle_f32({k: (v.double() if v.is_floating_point() else v) for k, v in d.items()}, sym)
        assert float((o64 - r['y']).abs().max()) < 1e-13 * max(top, 1.0)
        bound = sc.fused_bound(dt, it, p['roll'], d, r)
        assert bound.shape == r['y'].shape == (B, p['Ho'], p['Wo'], C) and float(bound.min()) > 0.0
        y, v = sc.emulate(dt, it, p['roll'], d, sym)
        emu = _ratio(y, r['y'], bound)
        assert emu < 1.0, (case, sym, emu)
        defects = {}
        for defect in sc.DEFECTS:
            bad = sc.ref(d, sym, defect=defect)
            if bad is not None:
                defects[defect] = _ratio(bad['y'], r['y'], bound)
                assert defects[defect] > 1.0, (case, sym, defect, defects[defect])
        assert sc.DEFECTS[1] in defects and sc.DEFECTS[2] in defects
        # pool rows: what the kernel adds (the rolling form: before the final rounding) is within the bound of the sums of the stored
        # output; a row that misses its last pixel is not
        good, pb = sc.pool_rows(y, p), sc.pool_bound(dt, y, p)
        assert bool(((sc.pool_rows(v, p) - good).abs() <= pb).all()), (case, sym)
        short = (sc.pool_rows(y, p, drop_last=True) - good).abs()
        assert bool((short > pb).any()), (case, sym)
        defects['a pool row missing its last pixel'] = float((short / pb).max())
        out.append((sym, emu, defects))
    assert out
    return out


@pytest.mark.parametrize('case', sc.FUSED_CASES, ids=[sc.case_id(c) for c in sc.FUSED_CASES])
def test_fused_reference_emulation_and_defects(lib, case):
    for sym, emu, defects in fused_ratios(lib, case):
        print('stem %s | pad %-4s | emulation / bound %.3f | defects / bound %s' % (
            sc.case_id(case), "''" if sym else 'same', emu, ', '.join('%.3g' % v for v in defects.values())))


@pytest.mark.parametrize('case', sc.UNFUSED_CASES, ids=[sc.unfused_id(c) for c in sc.UNFUSED_CASES])
def test_unfused_reference_emulation_and_defects(case):
    dt, it, C, H, W = case
    d = sc.unfused_inputs(case)
    seen = set()
    for sym in (False, True):
        r = sc.ref(d, sym, fused=False)
        top = float(r['e'].abs().max())
        assert float((sc.oracle_f32(d, sym, fused=False).double() - r['e']).abs().max()) < sc.F32_TOL * top
        o64 = sc.oracle_f32({k: (v.double() if v.is_floating_point() else v) for k, v in d.items()}, sym, fused=False)
        assert float((o64 - r['e']).abs().max()) < 1e-13 * max(top, 1.0)
        bound = sc.unfused_bound(dt, it, r)
        emu = _ratio(sc.emulate(dt, it, 0, d, sym, fused=False)[0], r['e'], bound)
        assert emu < 1.0, (case, sym, emu)
        for defect in (sc.DEFECTS[0], sc.DEFECTS[2]):
            bad = sc.ref(d, sym, defect=defect, fused=False)
            if bad is not None:
                seen.add(defect)
                assert _ratio(bad['e'], r['e'], bound) > 1.0, (case, sym, defect)
    assert sc.DEFECTS[2] in seen

