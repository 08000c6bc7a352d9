"""The three kernels an image enters the network through - the fused stem + stage-0 depthwise in its tile form (csrc/stem_dw.hip) and
its rolling-window form (csrc/stem_roll.hip), the unfused effdet_stem_conv[_u8] (csrc/dwconv.hip) - on the cases of
tests/_stem_cases.py (the table, the references and the separation of the bounds below are checked on the host by
test_stem_forms_host.py).

Per fused case and pad convention the entry accepts: |got - R64| within the per-element bound of _stem_cases.fused_bound (float32
2e-5 max |R64|, two-term 4e-5 max |R64|, bf16 the worst-case sum of the roundings the form makes, u = 2^-8), all finite; every pool
partial row written and within _stem_cases.pool_bound of the float64 sums of the output the kernel stored, partitioned by the plan.
Bit-exact: outputs and pool partials sit between sentinel NaNs and nothing else changes; a second run equals the first; each image
equals the same image run alone (B = 10: images 0, 7, 8, 9); without pool partials the output is the same.  The unfused conv: the
same without pools.  What the entry refuses returns EFFDET_EINVAL and touches nothing."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import _stem_cases as sc
from test_dwconv_forms_gpu import DEV, F32_SENT, SENT, Buf, _values


def _consts():
    m, s = sc.norm_consts()
    return (ctypes.c_float * 3)(*m.tolist()), (ctypes.c_float * 3)(*s.tolist())


def _wk(w, dtype):
    """[C, 3, 3, 3] -> [C][32] im2col weights, k = (ky * 3 + kx) * 3 + ci, in the weight dtype of the network dtype"""
    wk = torch.zeros(w.shape[0], 32)
    wk[:, :27] = w.permute(0, 2, 3, 1).reshape(w.shape[0], 27)
    return (wk.bfloat16() if dtype == 1 else wk).contiguous().to(DEV)


def _line_ok(got, r64, bound):
    ratio = (got - r64).abs() / bound
    return float(ratio.max()), float((got - r64).abs().max()) / float(r64.abs().max())


@pytest.mark.parametrize('case', sc.FUSED_CASES, ids=[sc.case_id(c) for c in sc.FUSED_CASES])
def test_stem_fused_form(case):
    from ood_object_detection_amd import _lib
    lib = _lib.load()
    dt, it, C, H, W, B = case
    d = sc.fused_inputs(case)
    x = d['raw'].contiguous().to(DEV)
    dev = [_wk(d['w'], dt)] + [t.contiguous().to(DEV) for t in (d['s1'], d['t1'], d['taps'].permute(2, 3, 0, 1).reshape(9, C), d['s2'], d['t2'])]
    cm, cs = _consts()
    st = torch.cuda.current_stream().cuda_stream
    Ho, Wo = (H + 1) // 2, (W + 1) // 2

    def run(first, nimg, sym, parts, pooled=True):
        y = Buf(SENT[dt], nimg, Ho * Wo * C)
        part = Buf(F32_SENT, nimg, parts * C) if pooled else None
        xi = x if nimg == B else x[first:first + nimg].clone()
        tail = [t.data_ptr() for t in dev] + [y.ptr(), part.ptr() if pooled else None, nimg, H, W, C]
        if it == 2:
            rc = lib.effdet_stem_dw_fused_u8(st, dt | (sc.PAD if sym else 0), xi.data_ptr(), cm, cs, *tail)
        else:
            rc = lib.effdet_stem_dw_fused(st, it, dt | (sc.PAD if sym else 0), xi.data_ptr(), *tail)
        assert rc == 0, rc
        torch.cuda.synchronize()
        return y, part

    ran = 0
    for sym in (False, True):
        p = sc.case_plan(lib, case, sym)
        assert (p is None) == sc.refused(case, sym)
        if p is None:
            continue
        ran += 1
        r = sc.ref(d, sym)
        bound = sc.fused_bound(dt, it, p['roll'], d, r)
        (y, part), (y2, part2) = run(0, B, sym, p['parts']), run(0, B, sym, p['parts'])
        got = _values(y.rows(), dt, (B, Ho, Wo, C))
        worst, rel = _line_ok(got, r['y'], bound)
        rows = part.rows().cpu().double().reshape(B, p['parts'], C)
        perr, pb = (rows - sc.pool_rows(got, p)).abs(), sc.pool_bound(dt, got, p)
        line = 'stem %s | pad %-4s | %s %dx%d parts of %dx%d | error %.3e of max |R64| | error / bound %.3f | pool error / bound %.3f' % (
            sc.case_id(case), "''" if sym else 'same', 'roll' if p['roll'] else 'tile', p['ny'], p['nx'], p['bh'], p['bw'], rel, worst, float((perr / pb).max()))
        print(line)
        assert bool(torch.isfinite(got).all()), line
        assert worst <= 1.0, line
        assert bool(torch.isfinite(rows).all()), 'a pool partial row was not written: ' + line
        assert bool((perr <= pb).all()), line
        for a, b in ((y, y2), (part, part2)):
            assert a.untouched() and b.untouched(), 'a launch wrote outside its rows: ' + line
            assert torch.equal(a.bits(), b.bits()), 'two runs differ: ' + line
        for i in (range(B) if B <= 2 else (0, 7, 8, 9)):
            one = run(i, 1, sym, p['parts'])
            for a, b in zip((y, part), one):
                assert b.untouched(), 'a launch wrote outside its rows: ' + line
                assert torch.equal(a.bits()[i], b.bits()[0]), 'image %d differs between B = 1 and B = %d: %s' % (i, B, line)
        bare, _ = run(0, B, sym, p['parts'], pooled=False)
        assert bare.untouched() and torch.equal(y.bits(), bare.bits()), 'the output differs without pool partials: ' + line
    assert ran


@pytest.mark.parametrize('case', sc.UNFUSED_CASES, ids=[sc.unfused_id(c) for c in sc.UNFUSED_CASES])
def test_stem_conv_form(case):
    from ood_object_detection_amd import _lib
    lib = _lib.load()
    dt, it, C, H, W = case
    B = 2
    d = sc.unfused_inputs(case)
    x = d['raw'].contiguous().to(DEV)
    dev = [t.contiguous().to(DEV) for t in (d['w'].permute(2, 3, 1, 0).reshape(27, C), d['s1'], d['t1'])]
    cm, cs = _consts()
    st = torch.cuda.current_stream().cuda_stream
    Ho, Wo = (H + 1) // 2, (W + 1) // 2

    def run(first, nimg, sym):
        y = Buf(SENT[dt], nimg, Ho * Wo * C)
        xi = x if nimg == B else x[first:first + nimg].clone()
        tail = [t.data_ptr() for t in dev] + [y.ptr(), nimg, H, W, C]
        if it == 2:
            rc = lib.effdet_stem_conv_u8(st, dt | (sc.PAD if sym else 0), xi.data_ptr(), cm, cs, *tail)
        else:
            rc = lib.effdet_stem_conv(st, it, dt | (sc.PAD if sym else 0), xi.data_ptr(), *tail)
        assert rc == 0, rc
        torch.cuda.synchronize()
        return y

    for sym in (False, True):
        r = sc.ref(d, sym, fused=False)
        bound = sc.unfused_bound(dt, it, r)
        y, y2 = run(0, B, sym), run(0, B, sym)
        got = _values(y.rows(), dt, (B, Ho, Wo, C))
        worst, rel = _line_ok(got, r['e'], bound)
        line = 'stem_conv %s | pad %-4s | error %.3e of max |R64| | error / bound %.3f' % (sc.unfused_id(case), "''" if sym else 'same', rel, worst)
        print(line)
        assert bool(torch.isfinite(got).all()), line
        assert worst <= 1.0, line
        assert y.untouched() and y2.untouched(), 'a launch wrote outside its rows: ' + line
        assert torch.equal(y.bits(), y2.bits()), 'two runs differ: ' + line
        for i in range(B):
            one = run(i, 1, sym)
            assert one.untouched() and torch.equal(y.bits()[i], one.bits()[0]), 'image %d differs between B = 1 and B = %d: %s' % (i, B, line)


def test_stem_refusals():
    """EFFDET_EINVAL before any launch, the sentinel buffers untouched; the unfused conv refuses a bf16 image into the two-term dtype
    and a width off 8"""
    from ood_object_detection_amd import _lib
    lib = _lib.load()
    cm, cs = _consts()
    st = torch.cuda.current_stream().cuda_stream
    z = torch.zeros(128 * 32, device=DEV)                            # stands for every weight and per-channel vector
    xbuf = torch.zeros(2 * 3 * 64 * 64 + 4, device=DEV)              # any image of the list, with room for the byte offset

    def whole(b):
        return bool((b.buf.view(b.it) == b.pattern).all())

    for dt, it, C, H, W, sym, off, why in sc.REFUSALS:
        y, part = Buf(SENT[dt], 2, 8 * 16 * 72), Buf(F32_SENT, 2, 16 * 72)
        flag = dt | (sc.PAD if sym else 0)
        tail = [z.data_ptr()] * 6 + [y.ptr(), part.ptr(), 2, H, W, C]
        if it == 2:
            rc = lib.effdet_stem_dw_fused_u8(st, flag, xbuf.data_ptr() + off, cm, cs, *tail)
        else:
            rc = lib.effdet_stem_dw_fused(st, it, flag, xbuf.data_ptr() + off, *tail)
        torch.cuda.synchronize()
        assert rc == sc.EINVAL, (why, rc)
        assert whole(y) and whole(part), why
    for dt, it, C, why in ((2, 1, 32, 'bf16 image into two-term'), (1, 0, 12, 'Cout % 8'), (0, 0, 0, 'Cout = 0')):
        y = Buf(SENT[dt], 2, 8 * 16 * 72)
        rc = lib.effdet_stem_conv(st, it, dt, xbuf.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), y.ptr(), 2, 16, 32, C)
        torch.cuda.synchronize()
        assert rc == sc.EINVAL, (why, rc)
        assert whole(y), why
    assert lib.effdet_stem_dw_fused(st, 2, 1, xbuf.data_ptr(), *([z.data_ptr()] * 6), z.data_ptr(), None, 1, 16, 32, 32) == sc.EINVAL    # uint8 has its own entry
