"""The inference 1x1-conv GEMM (csrc/pw_gemm.hip) in float32, bf16 and two-term bf16, one case per form the networks use and per
named edge of tests/_pw_gemm_cases.py (the table, its classes, the references and the separation of the bounds below are checked
on the host by test_pw_gemm_forms_host.py).

Per case |got - R64| stays within the bound of _pw_gemm_cases.bound(): 2e-5 max |R64| in float32, 4e-5 max |R64| in the two-term
dtype, and in bf16 2 e_q max |R64| with e_q the error of the bf16-rounded float64 reference - measured from the references alone;
the factor 2 is for a float32 accumulation that lands on the other side of a bf16 rounding tie.  A gated bf16 call adds
2^-9 sum_k |a g w| |scale| element by element: the kernel folds the gate into W and rounds w g to bf16, a second rounding inside
the sum that the reference (gate applied to unrounded products) does not make.
Bit-exact: the output sits in a buffer of sentinel NaNs - before, after and, when ldc > N or the image stride has slack, between
the rows - and nothing but the rows changes; each image of the batch equals the same image run alone (workgroups never straddle
images; for the large form this is also the 256-thread kernel against the 512-thread one); a second run equals the first; a group
launch equals the single launches of its problems, in both forms."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import _pw_gemm_cases as pc
import _pw_gemm_ref as pr

DEV = 'cuda:0'
SINGLE = [c for c in pc.CASES if len(c) != 4]
GROUPS = [c for c in pc.CASES if len(c) == 4]
SENT = {0: (torch.float32, torch.int32, 0x7FC5A5A5), 1: (torch.bfloat16, torch.int16, 0x7FC5), 2: (torch.float32, torch.int32, 0x7FC5A5A5)}


class Out:
    """[guard | B images, `slot` elements apart | guard] filled with NaNs no kernel computes; a row owns N elements at ldc.  A batch
    launch has slot = c_image_stride; launches of single images go side by side into one buffer whose slots keep a guard between
    them and the alignment of the whole"""

    def __init__(self, dtype, B, rpi, N, ldc, cis, side_by_side=False):
        self.tt, self.it, self.pattern = SENT[dtype]
        self.dtype, self.B, self.rpi, self.N, self.ldc, self.cis = dtype, B, rpi, N, ldc, cis
        self.slot = (cis + 15) // 16 * 16 + pc.GUARD if side_by_side else cis
        self.buf = torch.full((2 * pc.GUARD + B * self.slot,), self.pattern, dtype=self.it, device=DEV).view(self.tt)

    def ptr(self, image=0):
        return self.buf.data_ptr() + (pc.GUARD + image * self.slot) * self.buf.element_size()

    def _images(self, t):
        """[B, rpi, N] strided view of the rows of t (laid out as buf)"""
        return t[pc.GUARD:].as_strided((self.B, self.rpi, self.N), (self.slot, self.ldc, 1))

    def rows(self):
        return self._images(self.buf)

    def bits(self):
        return self.rows().contiguous().view(self.it)

    def values(self):
        r = self.rows().contiguous().cpu()
        if self.dtype == 2:
            from ood_object_detection_amd import pairfmt
            return pairfmt.decode(r).double()
        return r.double()

    def untouched(self):
        own = torch.zeros(self.buf.numel(), dtype=torch.bool, device=DEV)
        self._images(own)[:] = True
        return bool((self.buf.view(self.it)[~own] == self.pattern).all())


def _store(x, dtype):
    """values already representable in the storage type -> the device tensor the kernel reads"""
    if x is None:
        return None
    if dtype == 2:
        from ood_object_detection_amd import pairfmt
        return pairfmt.encode(x).to(DEV)
    return x.to(torch.float32 if dtype == 0 else torch.bfloat16).to(DEV)


def _f32(x):
    return None if x is None else x.float().contiguous().to(DEV)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _launch(lib, dtype, dev, d, first, nimg, out, slot=0):
    """images [first, first + nimg) of the problem into image `slot` of out.  An image starts on a 16-byte boundary of A, and of the
    residual whenever the whole batch's rows are 16-byte multiples, so a part of the batch is as aligned as the whole."""
    rpi = d['rpi']
    es = dev['a'].element_size()
    K, N = dev['a'].shape[1], dev['w'].shape[0]
    rc = lib.effdet_pw_gemm_bn_act(torch.cuda.current_stream().cuda_stream, dtype, dev['a'].data_ptr() + first * rpi * K * es, nimg * rpi, K,
                                   dev['w'].data_ptr(), N, _ptr(dev['scale']), dev['shift'].data_ptr(), d['act'],
                                   None if dev['res'] is None else dev['res'].data_ptr() + first * rpi * N * es,
                                   None if dev['gate'] is None else dev['gate'].data_ptr() + first * K * 4, rpi,
                                   out.ptr(slot), d['cis'], d['ldc'])
    assert rc == 0, rc


def _device(d, dtype):
    return dict(a=_store(d['a'], dtype), w=_store(d['w'], dtype), res=_store(d['res'], dtype), gate=_f32(d['gate']),
                scale=_f32(d['scale']), shift=_f32(d['shift']))


def _check_error(dtype, d, p, got, what):
    r64 = pr.ref(d, p)
    bnd, e_q = pc.bound(dtype, d, r64)
    err = (got - r64).abs()
    ratio = float((err / bnd).max())
    line = 'pw_gemm form %s | e_q %s | error %.3e of max |R64| | error / bound %.3f' % (
        what, '-' if e_q is None else '%.3e' % e_q, float(err.max()) / float(r64.abs().max()), ratio)
    print(line)
    assert bool(torch.isfinite(got).all()), line
    assert ratio < 1.0 if dtype == 0 else ratio <= 1.0, line
    return line


@pytest.mark.parametrize('case', SINGLE, ids=[pc.case_id(c) for c in SINGLE])
def test_pw_gemm_form(case):
    from ood_object_detection_amd import _lib
    lib = _lib.load()
    name, dtype, B, rpi, K, N, gated, res, act, has_scale, lay = case
    p = pc.case_plan(lib, case)
    d = pc.make_inputs(case)
    if p is None:                                 # a launch the two-term dtype refuses (N % 8, an image stride off 32 bytes): -22, nothing written
        assert dtype == 2 and (N % 8 or lay == 'odd')
        dev = _device(dict(d, res=None), dtype)
        out = Out(dtype, B, rpi, N, d['ldc'], d['cis'])
        rc = lib.effdet_pw_gemm_bn_act(torch.cuda.current_stream().cuda_stream, dtype, dev['a'].data_ptr(), B * rpi, K, dev['w'].data_ptr(), N,
                                       _ptr(dev['scale']), dev['shift'].data_ptr(), act, None, _ptr(dev['gate']), rpi, out.ptr(), d['cis'], d['ldc'])
        torch.cuda.synchronize()
        assert rc == -22 and bool((out.buf.view(out.it) == out.pattern).all())
        return
    dev = _device(d, dtype)
    runs = []
    for _ in range(2):
        out = Out(dtype, B, rpi, N, d['ldc'], d['cis'])
        _launch(lib, dtype, dev, d, 0, B, out)
        runs.append(out)
    alone = Out(dtype, B, rpi, N, d['ldc'], d['cis'], side_by_side=True)
    for i in range(B):
        _launch(lib, dtype, dev, d, i, 1, alone, i)
    torch.cuda.synchronize()
    line = _check_error(dtype, d, p, runs[0].values().reshape(B * rpi, N), '%s %r' % (pc.case_id(case), pc.case_classes(lib, case)[0]))
    assert runs[0].untouched() and runs[1].untouched() and alone.untouched(), 'a launch wrote outside its rows: ' + line
    bits = runs[0].bits()
    assert torch.equal(bits, runs[1].bits()), 'two runs differ: ' + line
    same = (bits == alone.bits()).reshape(B, -1).all(1)
    assert bool(same.all()), 'images %s differ between B = 1 and B = %d: %s' % ((~same).nonzero().flatten().tolist()[:8], B, line)


@pytest.mark.parametrize('case', GROUPS, ids=[pc.case_id(c) for c in GROUPS])
def test_pw_gemm_group_form(case):
    from ood_object_detection_amd import _lib
    lib = _lib.load()
    name, dtype, problems, act = case
    plans = pc.case_plan(lib, case)
    ds = pc.make_inputs(case)
    devs = [_device(d, dtype) for d in ds]
    n = len(ds)
    arr = lambda ct, v: (ct * n)(*v)

    def group():
        outs = [Out(dtype, 1, M, N, N, M * N) for M, K, N, _ in problems]
        rc = lib.effdet_pw_gemm_group(torch.cuda.current_stream().cuda_stream, dtype, n, arr(ctypes.c_void_p, [v['a'].data_ptr() for v in devs]),
                                      arr(ctypes.c_longlong, [q[0] for q in problems]), arr(ctypes.c_int, [q[1] for q in problems]),
                                      arr(ctypes.c_void_p, [v['w'].data_ptr() for v in devs]), arr(ctypes.c_int, [q[2] for q in problems]),
                                      arr(ctypes.c_void_p, [_ptr(v['scale']) for v in devs]), arr(ctypes.c_void_p, [v['shift'].data_ptr() for v in devs]),
                                      act, arr(ctypes.c_void_p, [o.ptr() for o in outs]))
        assert rc == 0, rc
        torch.cuda.synchronize()
        return outs

    first, second = group(), group()
    classes = pc.case_classes(lib, case)
    for i, (d, dv, p, o, o2) in enumerate(zip(ds, devs, plans, first, second)):
        M, K, N, _ = problems[i]
        line = _check_error(dtype, d, p, o.values().reshape(M, N), '%s problem %d %r' % (pc.case_id(case), i, classes[i]))
        assert o.untouched() and o2.untouched(), 'a launch wrote outside its rows: ' + line
        assert torch.equal(o.bits(), o2.bits()), 'two runs differ: ' + line
        single = Out(dtype, 1, M, N, N, M * N)
        _launch(lib, dtype, dv, d, 0, 1, single)
        torch.cuda.synchronize()
        assert single.untouched() and torch.equal(o.bits(), single.bits()), 'the group launch differs from the single launch: ' + line
