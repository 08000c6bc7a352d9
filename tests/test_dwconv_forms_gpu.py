"""The unfused depthwise path of csrc/dwconv.hip - effdet_dwconv_bn_act, effdet_se_gate, effdet_maxpool_same - in float32, bf16 and
two-term bf16 on the cases of tests/_dwconv_cases.py (the table, the references and the separation of the bounds below are checked
on the host by test_dwconv_forms_host.py).

Depthwise conv, per case, pad convention and (act 1 with pool partial sums | act 0 without): max |got - R64| within 2e-5 max |R64|
in float32, 4e-5 max |R64| in the two-term dtype and 2 e_q max |R64| in bf16, e_q being the error of the bf16-rounded float64
reference - measured from the references alone; the factor 2 is for the float32 accumulation and the hardware exp2 of SiLU landing
on the other side of a bf16 rounding tie.  The pool partial sums are checked per workgroup against the float64 sums of the output
the kernel stored (what the next layer reads), within the float32 summation bound of _dwconv_cases.pool_bound().
SE gate: 2e-5 of max |ref| against the float64 gate (the figure of tests/test_kernels_gpu.py).  Max pool: equal to the reference
bit for bit (the maximum of stored values is a stored value).
Bit-exact: outputs and pool partials sit between sentinel NaNs (the max pool's also between its images) and nothing else changes;
each image equals the same image run alone; a second run equals the first."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import _dwconv_cases as dc

DEV = 'cuda:0'
GUARD = 64
SENT = {0: (torch.float32, torch.int32, 0x7FC5A5A5), 1: (torch.bfloat16, torch.int16, 0x7FC5), 2: (torch.float32, torch.int32, 0x7FC5A5A5)}
F32_SENT = (torch.float32, torch.int32, 0x7FC5A5A5)


class Buf:
    """[guard | nimg images of `stride` elements, the first `used` of each owned | guard] of sentinel NaNs"""

    def __init__(self, kind, nimg, used, stride=None):
        self.tt, self.it, self.pattern = kind
        self.nimg, self.used, self.stride = nimg, used, stride or used
        self.buf = torch.full((2 * GUARD + nimg * self.stride,), self.pattern, dtype=self.it, device=DEV).view(self.tt)

    def ptr(self):
        return self.buf.data_ptr() + GUARD * self.buf.element_size()

    def rows(self):
        return self.buf[GUARD:GUARD + self.nimg * self.stride].view(self.nimg, self.stride)[:, :self.used]

    def bits(self):
        return self.rows().contiguous().view(self.it)

    def untouched(self):
        own = torch.zeros(self.buf.numel(), dtype=torch.bool, device=DEV)
        own[GUARD:GUARD + self.nimg * self.stride].view(self.nimg, self.stride)[:, :self.used] = True
        return bool((self.buf.view(self.it)[~own] == self.pattern).all())


def _store(x, dtype):
    """NHWC values representable in the storage type -> device tensor"""
    if dtype == 2:
        from ood_object_detection_amd import pairfmt
        return pairfmt.encode(x).to(DEV)
    return x.to(torch.float32 if dtype == 0 else torch.bfloat16).contiguous().to(DEV)


def _values(rows, dtype, shape):
    r = rows.contiguous().cpu().reshape(shape)
    if dtype == 2:
        from ood_object_detection_amd import pairfmt
        return pairfmt.decode(r).double()
    return r.double()


@pytest.mark.parametrize('case', dc.DW_CASES, ids=[dc.case_id(c) for c in dc.DW_CASES])
def test_dwconv_form(case):
    from ood_object_detection_amd import _lib
    lib = _lib.load()
    dt, C, H, W, k, s = case
    Ho, Wo = (H + s - 1) // s, (W + s - 1) // s
    d = dc.dw_inputs(case)
    x = _store(d['x'].permute(0, 2, 3, 1).contiguous(), dt)
    taps = d['w'].permute(2, 3, 0, 1).reshape(k * k, C).contiguous().to(DEV)
    scale, shift = d['scale'].contiguous().to(DEV), d['shift'].contiguous().to(DEV)
    st = torch.cuda.current_stream().cuda_stream

    def run(first, nimg, sym, act, pooled, nblk):
        y = Buf(SENT[dt], nimg, Ho * Wo * C)
        part = Buf(F32_SENT, nimg, nblk * C) if pooled else None
        xi = x if nimg == dc.B else x[first:first + nimg].clone()
        rc = lib.effdet_dwconv_bn_act(st, dt | (dc.PAD if sym else 0), xi.data_ptr(), y.ptr(), taps.data_ptr(), scale.data_ptr(), shift.data_ptr(),
                                      act, part.ptr() if pooled else None, nimg, H, W, C, k, s)
        assert rc == 0, rc
        torch.cuda.synchronize()
        return y, part

    for sym in (False, True):
        for act, pooled in ((1, True), (0, False)):
            p = dc.case_plan(lib, case, pooled, sym)
            nblk = p['blocks']
            r64 = dc.dw_ref(case, d, sym, act)
            bnd, e_q = dc.dw_bound(dt, r64)
            (y, part), (y2, part2) = run(0, dc.B, sym, act, pooled, nblk), run(0, dc.B, sym, act, pooled, nblk)
            got = _values(y.rows(), dt, (dc.B, Ho, Wo, C))
            err = float((got - r64).abs().max())
            line = 'dwconv %s | pad %-4s | act %d | e_q %s | error %.3e of max |R64| | error / bound %.3f' % (
                dc.case_id(case), "''" if sym else 'same', act, '-' if e_q is None else '%.3e' % e_q, err / float(r64.abs().max()), err / bnd)
            if pooled:
                stored = got.reshape(dc.B, Ho * Wo, C)
                want, pb = dc.pool_blocks(stored, p['ppb'], nblk), dc.pool_bound(dt, stored, p['ppb'], nblk)
                perr = (part.rows().cpu().double().reshape(dc.B, nblk, C) - want).abs()
                line += ' | pool error / bound %.3f' % float((perr / pb).max())
            print(line)
            assert bool(torch.isfinite(got).all()), line
            assert (err < bnd) if dt == 0 else (err <= bnd), line
            if pooled:
                assert bool((perr <= pb).all()), line
            bufs, again = [y] + ([part] if pooled else []), [y2] + ([part2] if pooled else [])
            for a, b in zip(bufs, again):
                assert a.untouched() and b.untouched(), 'a launch wrote outside its rows: ' + line
                assert torch.equal(a.bits(), b.bits()), 'two runs differ: ' + line
            for i in range(dc.B):
                one = run(i, 1, sym, act, pooled, nblk)
                for a, b in zip(bufs, one):
                    assert b.untouched(), 'a launch wrote outside its rows: ' + line
                    assert torch.equal(a.bits()[i], b.bits()[0]), 'image %d differs between B = 1 and B = %d: %s' % (i, dc.B, line)


@pytest.mark.parametrize('C', dc.SE_C)
def test_se_gate_form(C):
    from ood_object_detection_amd import _lib
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    for nblk in dc.SE_NBLK:
        for R in dc.SE_R:
            d = dc.se_inputs(C, nblk, R)
            ref = dc.se_ref(d)
            dev = [t.contiguous().to(DEV) for t in (d['partial'], d['W1'], d['b1'], d['W2'].t(), d['b2'])]     # conv_expand goes in transposed
            outs = []
            for _ in range(2):
                gate = Buf(F32_SENT, dc.B, C)
                rc = lib.effdet_se_gate(st, dev[0].data_ptr(), nblk, d['hw'], dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(),
                                        dev[4].data_ptr(), gate.ptr(), dc.B, C, R)
                assert rc == 0, rc
                torch.cuda.synchronize()
                outs.append(gate)
            got = outs[0].rows().cpu().double()
            err = float((got - ref).abs().max()) / float(ref.abs().max())
            line = 'se_gate C %d nblk %d R %d | error %.3e of max |ref|' % (C, nblk, R, err)
            print(line)
            assert bool(torch.isfinite(got).all()) and err < dc.F32_TOL, line
            assert outs[0].untouched() and outs[1].untouched() and torch.equal(outs[0].bits(), outs[1].bits()), line
            for i in range(dc.B):
                one = Buf(F32_SENT, 1, C)
                pi = dev[0][i:i + 1].clone()
                assert lib.effdet_se_gate(st, pi.data_ptr(), nblk, d['hw'], dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(),
                                          dev[4].data_ptr(), one.ptr(), 1, C, R) == 0
                torch.cuda.synchronize()
                assert one.untouched() and torch.equal(outs[0].bits()[i], one.bits()[0]), 'image %d alone differs: %s' % (i, line)


@pytest.mark.parametrize('case', dc.POOL_CASES, ids=['%s-c%d-%dx%d-slack%d' % ((dc.DTYPE_NAME[c[0]],) + tuple(c[1:])) for c in dc.POOL_CASES])
def test_maxpool_form(case):
    """input and output image strides larger than the maps (slack elements of sentinel between the images)"""
    from ood_object_detection_amd import _lib
    lib = _lib.load()
    dt, C, H, W, slack = case
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    xv = dc.pool_inputs(case)
    xs = _store(xv, dt).reshape(dc.B, H * W * C)
    st = torch.cuda.current_stream().cuda_stream
    for sym in (False, True):
        ref = dc.pool_ref(xv, sym)
        outs = []
        for nimg, first in ((dc.B, 0), (dc.B, 0)) + tuple((1, i) for i in range(dc.B)):
            xin = Buf(SENT[dt], nimg, H * W * C, H * W * C + slack)
            xin.rows()[:] = xs[first:first + nimg]
            y = Buf(SENT[dt], nimg, Ho * Wo * C, Ho * Wo * C + slack)
            rc = lib.effdet_maxpool_same(st, dt | (dc.PAD if sym else 0), xin.ptr(), xin.stride if slack else 0, y.ptr(), y.stride if slack else 0,
                                         nimg, H, W, C)
            assert rc == 0, rc
            torch.cuda.synchronize()
            assert y.untouched() and xin.untouched(), case
            outs.append(y)
        got = _values(outs[0].rows(), dt, (dc.B, Ho, Wo, C))
        assert torch.equal(got, ref.double()), (case, sym, float((got - ref.double()).abs().max()))
        assert torch.equal(outs[0].bits(), outs[1].bits())
        for i in range(dc.B):
            assert torch.equal(outs[0].bits()[i], outs[2 + i].bits()[0]), (case, sym, i)
