"""Host checks behind tests/test_mbconv_variants_gpu.py (no GPU): the case table of tests/_mbconv_cases.py reaches every fused-MBConv
kernel class that the d0 ... d5 backbones run - asked of effdet_mbconv_plan_describe, i.e. of the launcher's own mbconv_plan() - and
the edge geometries of every (dtype, form); the cases are as small as their class allows; and on every case the yardstick of the
GPU test separates the float64 reference from one whose last output column reads a window shifted by one pixel."""
import collections
import ctypes

import pytest
import torch

import _mbconv_cases as mc
import _mbconv_ref as mr

IDS = ['%03d-%s' % (i, mc.case_id(c)) for i, c in enumerate(mc.CASES)]


@pytest.fixture(scope='module')
def lib():
    from ood_object_detection_amd import _lib
    return _lib.load()


@pytest.fixture(scope='module')
def used(lib):
    return mc.used_classes(lib)


def test_plan_query_contract(lib):
    """slot order, truncation to n, the pad flag is stripped, bad arguments"""
    out = (ctypes.c_int * mc.PLAN_INTS)()
    args = (1, 40, 40, 80, 480, 3, 1, 0)
    assert lib.effdet_mbconv_plan_describe(*args, out, mc.PLAN_INTS) == mc.PLAN_INTS
    full = list(out)
    p = dict(zip(mc.FIELDS, full))
    assert p['form'] == mc.WIDE and p['parts'] == p['nstrips'] * p['nbands'] and p['nkc'] == 3 and p['lds'] > 0
    assert p['nchunks'] == p['TH'] == p['TW'] == p['tiles_x'] == p['tiles_y'] == 0               # unused slots
    assert p['MT'] * 16 >= (p['TWo'] - 1) * 1 + 3 and p['NO'] == (p['TWo'] + 15) // 16
    for i in range(mc.PLAN_INTS):
        out[i] = -7
    assert lib.effdet_mbconv_plan_describe(*args, out, 5) == 5
    assert list(out)[:5] == full[:5] and all(v == -7 for v in list(out)[5:])
    assert lib.effdet_mbconv_plan_describe(args[0] | mc.PAD, *args[1:], out, mc.PLAN_INTS) == mc.PLAN_INTS and list(out) == full
    assert lib.effdet_mbconv_plan_describe(*args, None, mc.PLAN_INTS) == -22
    assert lib.effdet_mbconv_plan_describe(*args, out, 0) == -22
    for cin, mid in ((84, 480), (80, 484), (0, 480), (80, 0)):          # what the launcher refuses before it plans
        assert lib.effdet_mbconv_plan_describe(1, 40, 40, cin, mid, 3, 1, 0, out, mc.PLAN_INTS) == -22
    # a geometry no fused form takes (two-term bf16, input wider than 192 channels): form 0, every slot 0
    assert lib.effdet_mbconv_plan_describe(2, 20, 20, 320, 1920, 3, 1, 0, out, mc.PLAN_INTS) == mc.PLAN_INTS and not any(out)
    assert lib.effdet_mbconv_tiles_per_image(2, 20, 20, 320, 1920, 3, 1) == -22
    # deep and front fill their own slots
    d = mc.plan(lib, 0, 0, 192, 1152, 20, 20, 5, 1)
    assert d['form'] == mc.DEEP and d['nchunks'] == 18 and d['parts'] == d['nbands'] and d['band_rows'] * d['nbands'] >= 20 and d['MT'] == 0
    f = mc.plan(lib, 0, 0, 16, 96, 64, 64, 3, 2)
    assert f['form'] == mc.FRONT and f['parts'] == f['tiles_x'] * f['tiles_y'] and f['tiles_x'] == (32 + f['TW'] - 1) // f['TW'] and f['nbands'] == 0


def test_every_used_class_has_a_case(lib, used):
    """every class of every swept block has a case whose own plan has that class: the share of used classes left out is zero"""
    have = collections.Counter()
    for case in mc.CASES:
        got = mc.case_class(lib, case)
        assert got == case[8], ('the case no longer reaches the class it is in the table for', case, got)
        have[got] += 1
    counts = collections.Counter((c[0], c[2]) for c in used)
    for (dt, form), n in sorted(counts.items()):
        print('%-14s %-5s %3d classes used by the backbones, %3d cases' %
              (mc.DTYPE_NAME[dt], mc.FORM_NAME[form], n, sum(1 for c in mc.CASES if (c[0], c[8][2]) == (dt, form))))
    print('total %d classes, %d cases' % (len(used), len(mc.CASES)))
    missing = sorted(c for c in used if not have[c])
    assert not missing, ['%r, e.g. %r' % (c, used[c]) for c in missing]
    assert all(c[8][2] != mc.NONE for c in mc.CASES)
    assert dict(counts) == mc.CLASS_COUNTS                     # the counts DESIGN.md records


def test_edge_geometries(lib, used):
    """per (dtype, form) in use: a ragged last strip / tile column, a ragged last band / tile row, odd H and W, and stride 2 on an
    even and on an odd map (the deep form has no column split: its bands span whole rows)"""
    plans = [(c, mc.case_plan(lib, c)) for c in mc.CASES]
    for dt, form in sorted({(c[0], c[2]) for c in used}):
        for name, applies, holds in mc.EDGES:
            if not applies(form):
                continue
            hits = [c for c, p in plans if c[0] == dt and p['form'] == form and holds(p, c)]
            assert hits, (mc.DTYPE_NAME[dt], mc.FORM_NAME[form], name)
    for c, p in plans:                                          # a case listed for an edge has it
        for name in c[9]:
            holds = [e[2] for e in mc.EDGES if e[0] == name]
            assert len(holds) == 1 and holds[0](p, c), (c, name)


def test_parts_agree(lib):
    """`parts` of the plan is what effdet_mbconv[_gated]_tiles_per_image answers, on every case and every swept block"""
    blocks = [b[2:] for b in mc.swept_blocks()] + [c[:8] for c in mc.CASES]
    for dt, gated, Cin, mid, H, W, k, s in blocks:
        p = mc.plan(lib, dt, gated, Cin, mid, H, W, k, s)
        fn = lib.effdet_mbconv_gated_tiles_per_image if gated else lib.effdet_mbconv_tiles_per_image
        for flag in (0, mc.PAD):
            t = fn(dt | flag, H, W, Cin, mid, k, s)
            assert (t == p['parts'] and t > 0) if p['form'] != mc.NONE else (t == -22 and p['parts'] == 0), (dt, gated, Cin, mid, H, W, k, s, t, p)


def _serves(lib, case, H, W):
    """does the (H, W) problem with the case's channels reach the case's class and the edge geometries it is listed for?"""
    c = case[:4] + (H, W) + case[6:]
    p = mc.case_plan(lib, c)
    holds = {e[0]: e[2] for e in mc.EDGES}
    return mc.klass(p, c[0], c[1], c[6], c[7]) == case[8] and all(holds[n](p, c) for n in case[9])


def test_cases_are_small(lib):
    """B * Ho * Wo * mid <= 4e6; H and W are no larger than the class (and the case's edge geometry) needs: the same problem one
    or two rows / columns smaller - down to 2k + 1, or to the sweep's smallest map where nothing that large serves - no longer serves; mid = 6 * Cin (the composed first block keeps its own 3 * Cin)"""
    for case in mc.CASES:
        dt, gated, Cin, mid, H, W, k, s = case[:8]
        Ho, Wo = mc.same_out(H, s), mc.same_out(W, s)
        assert mc.B * Ho * Wo * mid <= mc.MAX_ELEMS, case
        lo = mc.floor(k)
        if H < lo or W < lo:                                      # a class that only maps below 2k + 1 reach: none up to 3k serves
            assert min(H, W) >= mc.SMALLEST and not any(_serves(lib, case, h, w) for h in range(lo, 3 * k + 1) for w in range(lo, 3 * k + 1)), case
            lo = mc.SMALLEST
        assert mid == 6 * Cin or (gated and mid == 3 * Cin), case
        for d in (1, 2):
            assert H - d < lo or not _serves(lib, case, H - d, W), ('H could be %d' % (H - d), case)
            assert W - d < lo or not _serves(lib, case, H, W - d), ('W could be %d' % (W - d), case)
        if case[8][2] == mc.ROLL and not case[9]:
            assert Ho < 80, case                                  # (roll bands are 40+ rows: only the several-bands edge needs them)
    assert len(set((c[:8], c[9]) for c in mc.CASES)) == len(mc.CASES)


def test_bf16_element_bound_needs_the_half_ulp():
    """why the bf16 element bound is not the pooled bound's formula taken literally: with 2^-9 |ref| for the final rounding, the
    float64 reference itself, correctly rounded to bf16, lies outside on an element where BN2's shift dominates the taps (0.3155
    stores as 0.3164: 3.0e-3 of the value, half a unit in the last place of the binade [0.25, 0.5)).  With the exact half-ulp the
    same element sits on the bound's rounding term and inside the bound."""
    case = next(c for c in mc.CASES if c[:8] == (1, 0, 24, 144, 7, 47, 3, 1))
    d = mr.make_inputs(case, mc.B)
    ref, amp, _ = mr.reference(case, d)
    stored = mr.quantize(ref.permute(0, 2, 3, 1).float(), 1).permute(0, 3, 1, 2).double()
    err = (stored - ref).abs()
    literal = 2.0 ** -9 * (2 * 1.1 * amp[0] + ref.abs()) + 1e-5
    assert float((err / literal).max()) > 1.0
    assert bool((err <= mr.half_ulp_bf16(ref) * (1 + 1e-6)).all())
    hu = mr.half_ulp_bf16(ref)
    assert bool((hu >= 2.0 ** -9 * ref.abs()).all()) and bool((hu <= 2.0 ** -8 * ref.abs()).all())
    assert float((err / mr.bound(case, ref, amp)).max()) < 1.0


@pytest.mark.parametrize('case', mc.CASES, ids=IDS)
def test_yardstick_separates_a_shifted_last_column(case):
    """on the GPU test's own inputs: the reference whose last output column reads a window shifted by one input pixel breaks the
    yardstick on at least one element, the correct reference rounded to the storage dtype stays inside - under TF-SAME padding and,
    for the stride-2 cases (which the GPU test also runs with symmetric padding), under symmetric padding"""
    d = mr.make_inputs(case, mc.B)
    e = None
    for pad in ('same', '') if case[7] == 2 else ('same',):
        ref, amp, e = mr.reference(case, d, pad, e)
        bnd = mr.bound(case, ref, amp)
        stored = mr.quantize(ref.permute(0, 2, 3, 1).float(), case[0]).permute(0, 3, 1, 2).double()
        inside, _ = mr.worst((stored - ref).abs(), bnd)
        bad = mr.wrong_reference(case, d, ref, e, pad)
        outside, where = mr.worst((bad - ref).abs(), bnd)
        assert where[3] == ref.shape[3] - 1
        assert inside < 1.0, (pad, inside)
        assert outside > 1.0, (pad, outside)
        frac = float(((bad - ref).abs() > bnd)[..., -1].double().mean())
        assert frac > 0.5, (pad, frac)                            # not one lucky element: most of the column is visibly wrong
