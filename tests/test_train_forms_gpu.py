"""Every kernel class of the training GEMMs and depthwise entries of csrc/train_net.hip that the d0 ... d5 training step runs
(the case table of tests/_train_cases.py; tests/test_train_forms_host.py proves it leaves none out), each case twice:

exact  every operand is a seeded integer of magnitude 1 ... 3, so every linear output must EQUAL the int64 reference - no tolerance;
real   _seeded.seeded_array operands against float64 at the yardsticks the older tests use for the same quantity:
       2e-6 sqrt(K) (gemm_nt), 3e-6 sqrt(M) (gemm_tn), 1e-5 (depthwise Z, dX), 2e-5 (tap gradients, sum of dY), of the largest entry.
Outputs that pass through silu_train / silu_grad get no tolerance of their own: they are compared with the function applied in
float64 to the kernel's OWN linear output at the yardstick of test_elementwise_family (1e-6 silu, 2e-6 its gradient), and the pool
partial rows summed over the blocks with the sum of the kernel's own A at 1e-5.  Outputs and the workspace are NaN before the
launch, outputs sit between guard regions that must come back untouched, and so must the gap columns of a strided row map."""
import ctypes
import math

import pytest
import torch

import _train_cases as tc
import _train_ref as tr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 256                                           # floats before and after every output
SENTINEL = 12345.0
IDS = ['%03d-%s' % (i, tc.case_id(c)) for i, c in enumerate(tc.CASES)]
FIRST = {}                                            # class -> its first case: the one that also runs twice, bit-equal
for _c in tc.CASES:
    FIRST.setdefault(_c[-2], _c)


@pytest.fixture(scope='module')
def lib():
    from ood_object_detection_amd import _lib
    return _lib.load()


def _stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


class _Buf(object):
    """a float32 device array at a chosen address mod 16, between two guard regions, inside a larger allocation"""

    def __init__(self, n, align=0, init=None):
        self.n = int(n)
        self.base = torch.full((2 * GUARD + self.n + 4,), SENTINEL, dtype=torch.float32, device=DEV)
        assert self.base.data_ptr() % 16 == 0 and align % 4 == 0
        self.off = GUARD + align // 4
        self.view = self.base[self.off:self.off + self.n]
        self.view.copy_(init.reshape(-1)) if init is not None else self.view.fill_(float('nan'))
        assert self.view.data_ptr() % 16 == align

    @property
    def ptr(self):
        return self.view.data_ptr()

    def cpu(self):
        assert bool((self.base[:self.off] == SENTINEL).all()) and bool((self.base[self.off + self.n:] == SENTINEL).all()), 'guard overwritten'
        return self.view.cpu()


def _in(t, align=0):
    return None if t is None else _Buf(t.numel(), align, t)


def _ptr(b):
    return None if b is None else b.ptr


def _close(got, ref, rtol, what):
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), '%s: not every element was written' % what
    err = float((got - ref).abs().max())
    lim = rtol * max(float(ref.abs().max()), 1e-6)
    print('%s: L-inf %.3e, limit %.3e' % (what, err, lim))
    assert err <= lim, '%s: L-inf %.3e > %.3e (max|ref| %.3e)' % (what, err, lim, float(ref.abs().max()))


def _equal(got, ref, what):
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = (got != ref) | ~torch.isfinite(got)
    assert not bool(bad.any()), '%s: %d of %d elements differ from the integer reference, first at %r' % (
        what, int(bad.sum()), bad.numel(), tuple(int(v) for v in bad.nonzero()[0]))


def _check(mode, got, ref, rtol, what):
    _equal(got, ref, what) if mode == 'exact' else _close(got, ref, rtol, what)


def _levels_args(lv):
    B, hw = lv
    L = len(hw)
    return B, L, (ctypes.c_int * L)(*[h for h, _ in hw]), (ctypes.c_int * L)(*[w for _, w in hw])


# ---- gemm_nt --------------------------------------------------------------------------------------------------------
def run_nt(lib, case, d):
    """-> (C [M, N], C2 or None) as the kernel wrote them (CPU); checks guards and the gap columns of a non-dense C"""
    from ood_object_detection_amd import _lib
    _, entry, M, K, N, akind, ckind, pk, lv, ops, rows, align = case[:12]
    a_al, w_al, c_al, b_al, r_al, c2_al, g_al, m_al = align
    if akind == tc.DENSE:
        A = _in(d['A'], a_al)
    else:
        A = _in(tr.place(case, d['A'], K)[0].nan_to_num(nan=SENTINEL), a_al)       # the rows between the mapped ones are never read
    W, bias, gate = _in(d['W'], w_al), _in(d.get('bias'), b_al), _in(d.get('gate'), g_al)
    start = None
    if ckind == tc.DENSE:
        nC = M * N

        def lay(t):
            return t
    else:
        nC = tc.packed_floats(case)

        def lay(t):
            return None if t is None else tr.place(case, t, N)[0]
        start = tr.place(case, None, N)[1]
    C = _Buf(nC, c_al, lay(d.get('prev')))
    R, mask = _in(lay(d.get('R')), r_al), _in(lay(d.get('mask')), m_al)
    C2 = _Buf(nC, c2_al) if ops & tc.C2 else None
    st = _stream()
    if entry == 'gemm_nt':
        am = pk if akind == tc.STRIDED else (0, 0, 0)
        cm = pk if ckind == tc.STRIDED else (0, 0, 0)
        rc = lib.effdet_train_gemm_nt(st, A.ptr, am[0], am[1], am[2], W.ptr, _ptr(bias), C.ptr, cm[0], cm[1], cm[2], M, K, N,
                                      int(bool(ops & tc.ACC)), _ptr(C2))
    elif entry == 'gemm_nt_fused':
        rc = lib.effdet_train_gemm_nt_fused(st, A.ptr, _ptr(gate), rows, W.ptr, _ptr(bias), _ptr(R), C.ptr, _ptr(C2), M, K, N)
    elif entry == 'gemm_nt_relu':
        rc = lib.effdet_train_gemm_nt_relu(st, A.ptr, W.ptr, C.ptr, M, K, N)
    elif entry == 'gemm_nt_mask':
        rc = lib.effdet_train_gemm_nt_mask(st, A.ptr, W.ptr, mask.ptr, C.ptr, M, K, N)
    else:
        B, L, Hs, Ws = _levels_args(lv)
        rc = lib.effdet_train_gemm_nt_levels(st, A.ptr, int(akind == tc.LEVELS), W.ptr, _ptr(bias), C.ptr, int(ckind == tc.LEVELS), B, L, Hs, Ws,
                                             pk[1], pk[2], K, N, _ptr(C2))
    _lib.check(rc, entry)
    torch.cuda.synchronize()
    for b in (A, W, bias, gate, R, mask):
        if b is not None:
            b.cpu()                                     # guards of the inputs too
    out = []
    for b in (C, C2):
        if b is None:
            out.append(None)
            continue
        flat = b.cpu()
        if start is None:
            out.append(flat.reshape(M, N))
            continue
        out.append(tr.gather(flat, start, N))
        rest = flat.clone()
        rest[(start[:, None] + torch.arange(N)[None, :]).reshape(-1)] = float('nan')
        assert bool(torch.isnan(rest).all()), 'elements outside the mapped rows and columns were written'
    return out


@pytest.mark.parametrize('mode', ['exact', 'real'])
@pytest.mark.parametrize('case', [c for c in tc.CASES if c[0] == 'nt'], ids=[i for i, c in zip(IDS, tc.CASES) if c[0] == 'nt'])
def test_gemm_nt_forms(lib, case, mode):
    d = tr.operands(case, mode)
    ref = tr.nt_reference(case, d)
    C, C2 = run_nt(lib, case, d)
    _check(mode, C, ref, 2e-6 * math.sqrt(case[3]), 'C')
    if C2 is not None:
        _close(C2, tr.silu64(C), 1e-6, 'C2 against silu of the kernel\'s own C')


# ---- gemm_tn --------------------------------------------------------------------------------------------------------
def run_tn(lib, case, d):
    """-> (dW [N, K], dsum [N]) as the kernel wrote them (CPU)"""
    from ood_object_detection_amd import _lib
    _, entry, M, N, K, ykind, pk, lv, rows, align = case[:10]
    if ykind == tc.DENSE:
        dY = _in(d['dY'], align[0])
    else:
        dY = _in(tr.place(case, d['dY'], N)[0].nan_to_num(nan=SENTINEL), align[0])
    X, gate = _in(d['X'], align[1]), _in(d.get('gate'), align[2])
    nws = lib.effdet_train_gemm_tn_workspace_floats(M, N, K)
    assert nws > 0
    ws, out = _Buf(nws), _Buf(N * K + N)
    st = _stream()
    if entry == 'gemm_tn':
        ym = pk if ykind == tc.STRIDED else (0, 0, 0)
        rc = lib.effdet_train_gemm_tn(st, dY.ptr, ym[0], ym[1], ym[2], X.ptr, 0, 0, 0, M, N, K, out.ptr, ws.ptr, nws)
    elif entry == 'gemm_tn_scaled':
        rc = lib.effdet_train_gemm_tn_scaled(st, dY.ptr, X.ptr, gate.ptr, rows, M, N, K, out.ptr, ws.ptr, nws)
    else:
        B, L, Hs, Ws = _levels_args(lv)
        rc = lib.effdet_train_gemm_tn_levels(st, dY.ptr, int(ykind == tc.LEVELS), X.ptr, B, L, Hs, Ws, pk[1], pk[2], N, K, out.ptr, ws.ptr, nws)
    _lib.check(rc, entry)
    torch.cuda.synchronize()
    for b in (dY, X, gate):
        if b is not None:
            b.cpu()
    assert bool(torch.isfinite(ws.cpu()).all()), 'a partial row of the workspace was not written'
    o = out.cpu()
    return o[:N * K].reshape(N, K), o[N * K:]


@pytest.mark.parametrize('mode', ['exact', 'real'])
@pytest.mark.parametrize('case', [c for c in tc.CASES if c[0] == 'tn'], ids=[i for i, c in zip(IDS, tc.CASES) if c[0] == 'tn'])
def test_gemm_tn_forms(lib, case, mode):
    d = tr.operands(case, mode)
    ref_w, ref_s = tr.tn_reference(case, d)
    dW, dsum = run_tn(lib, case, d)
    rtol = 3e-6 * math.sqrt(case[2])
    _check(mode, dW, ref_w, rtol, 'dW')
    _check(mode, dsum, ref_s, rtol, 'dsum')
    if mode == 'real' and case is FIRST[case[-2]]:                    # the fixed summation order: bitwise the same again (one case per class)
        dW2, dsum2 = run_tn(lib, case, d)
        assert torch.equal(dW, dW2) and torch.equal(dsum, dsum2), 'two runs differ bitwise'


# ---- depthwise ------------------------------------------------------------------------------------------------------
def run_dw(lib, case, d):
    from ood_object_detection_amd import _lib
    _, which, B, H, W, C, k, s, pad, flag = case[:10]
    Ho, Wo = tc.same_out(H, s), tc.same_out(W, s)
    ksel = k | (tc.PAD if pad else 0)
    st = _stream()
    X, taps, dY = _in(d['X']), _in(d['taps']), _in(d['dY'])
    if which == 'fwd':
        scale, shift = _in(d['scale']), _in(d['shift'])
        nblk = lib.effdet_train_dwconv_fwd_parts(H, W, C, ksel, s)
        Z = _Buf(B * Ho * Wo * C)
        A = _Buf(B * Ho * Wo * C) if flag else None
        part = _Buf(B * nblk * C) if flag else None
        _lib.check(lib.effdet_train_dwconv_fwd(st, X.ptr, Z.ptr, _ptr(A), taps.ptr, scale.ptr, shift.ptr, _ptr(part), B, H, W, C, ksel, s),
                   'effdet_train_dwconv_fwd')
        torch.cuda.synchronize()
        return (Z.cpu().reshape(B, Ho, Wo, C), None if A is None else A.cpu().reshape(B, Ho, Wo, C),
                None if part is None else part.cpu().reshape(B, nblk, C))
    if which == 'bwd_dx':
        dX, dXz = _Buf(B * H * W * C), _Buf(B * H * W * C)
        Zb = _in(d['Zb'])
        _lib.check(lib.effdet_train_dwconv_bwd_dx(st, dY.ptr, taps.ptr, dX.ptr, B, H, W, C, ksel, s), 'effdet_train_dwconv_bwd_dx')
        if flag:
            _lib.check(lib.effdet_train_dwconv_bwd_dx_silu(st, dY.ptr, taps.ptr, Zb.ptr, dXz.ptr, B, H, W, C, ksel, s),
                       'effdet_train_dwconv_bwd_dx_silu')
        torch.cuda.synchronize()
        return dX.cpu().reshape(B, H, W, C), dXz.cpu().reshape(B, H, W, C) if flag else None
    nws = lib.effdet_train_dwconv_bwd_dw_workspace_floats(B, H, W, C, ksel, s)
    assert nws > 0
    ws, out = _Buf(nws), _Buf((k * k + 1) * C)
    _lib.check(lib.effdet_train_dwconv_bwd_dw(st, dY.ptr, X.ptr, out.ptr, B, H, W, C, ksel, s, ws.ptr, nws, int(flag)), 'effdet_train_dwconv_bwd_dw')
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ws.cpu()).all()), 'a partial row of the workspace was not written'
    o = out.cpu()
    dt = o[:k * k * C].reshape(C, k * k).t() if flag else o[:k * k * C].reshape(k * k, C)     # cmajor: the parameter's [C, k * k]
    return dt, o[k * k * C:]


@pytest.mark.parametrize('mode', ['exact', 'real'])
@pytest.mark.parametrize('case', [c for c in tc.CASES if c[0] == 'dw'], ids=[i for i, c in zip(IDS, tc.CASES) if c[0] == 'dw'])
def test_depthwise_forms(lib, case, mode):
    _, which, B, H, W, C, k, s, pad, flag = case[:10]
    d = tr.operands(case, mode)
    ref = tr.dw_reference(case, d)
    got = run_dw(lib, case, d)
    if which == 'fwd':
        Z, A, part = got
        _check(mode, Z, ref, 1e-5, 'Z')
        if flag:
            _close(A, tr.silu64(Z), 1e-6, 'A against silu of the kernel\'s own Z')
            _close(part.double().sum(1), A.double().sum((1, 2)), 1e-5, 'pool partial rows against the sum of the kernel\'s own A')
    elif which == 'bwd_dx':
        dX, dXz = got
        _check(mode, dX, ref, 1e-5, 'dX')
        if flag:
            _close(dXz, dX.double() * tr.silu_grad64(d['Zb']), 2e-6, 'dX with Z against the kernel\'s own dX times silu\'(Z)')
    else:
        dt, dsum = got
        _check(mode, dt, ref[0], 2e-5, 'tap gradients')
        _check(mode, dsum, ref[1], 2e-5, 'sum of dY')
        if mode == 'real' and case is FIRST[case[-2]]:                # the fixed summation order: bitwise the same again (one case per class)
            dt2, dsum2 = run_dw(lib, case, d)
            assert torch.equal(dt, dt2) and torch.equal(dsum, dsum2), 'two runs differ bitwise'


# ---- the sweep against a real step ----------------------------------------------------------------------------------
def test_sweep_covers_a_recorded_d0_step(lib, monkeypatch):
    """one tf_efficientdet_d0 training step at 128 px, 2 images, 20 classes with an _Ops subclass that records the arguments of
    every GEMM / depthwise call: the class of every recorded call (asked of the plan queries, with the real pointer alignment) is
    in the class set the sweep derives for that model, size and batch from the configs alone"""
    from ood_object_detection_amd import train_engine as te
    from ood_object_detection_amd.effdet.loss import DetectionLoss
    from test_train_gpu import _targets, _train_setup
    seen = []

    def al(*ts):
        return tuple(0 if t is None else t.data_ptr() % 16 for t in ts)

    class Recording(te._Ops):
        def gemm_nt(self, A, W, bias=None, M=None, a_map=None, out=None, c_map=None, silu_out=False):
            assert a_map is None and c_map is None
            N, K = W.shape
            r = super().gemm_nt(A, W, bias, silu_out=silu_out)
            c, c2 = r if silu_out else (r, None)
            seen.append(tc._nt('gemm_nt', A.numel() // K, K, N, (tc.BIAS if bias is not None else 0) | (tc.C2 if silu_out else 0),
                               align=al(A, W, c, bias, None, c2, None, None)))
            return r

        def gemm_nt_fused(self, A, W, bias=None, a_scale=None, a_rows=0, R=None, silu_out=False):
            N, K = W.shape
            r = super().gemm_nt_fused(A, W, bias, a_scale, a_rows, R, silu_out)
            c, c2 = r if silu_out else (r, None)
            ops = (tc.BIAS if bias is not None else 0) | (tc.RES if R is not None else 0) | (tc.C2 if silu_out else 0) | \
                  (tc.A_SCALE if a_scale is not None else 0)
            seen.append(tc._nt('gemm_nt_fused', A.numel() // K, K, N, ops, a_rows if a_scale is not None else 0,
                               align=al(A, W, c, bias, R, c2, a_scale, None)))
            return r

        def gemm_tn(self, dY, X, N, K, M=None, y_map=None, x_map=None, out=None):
            assert y_map is None and x_map is None
            seen.append(tc._tn('gemm_tn', dY.numel() // N, N, K, align=al(dY, X, None)))
            return super().gemm_tn(dY, X, N, K, out=out)

        def gemm_tn_scaled(self, dY, X, x_scale, x_rows, N, K, out=None):
            seen.append(tc._tn('gemm_tn_scaled', dY.numel() // N, N, K, x_rows, align=al(dY, X, x_scale)))
            return super().gemm_tn_scaled(dY, X, x_scale, x_rows, N, K, out=out)

        def gemm_nt_levels(self, lv, A, W, bias=None, a_packed=False, out_packed=None, pk=(0, 0)):
            N, K = W.shape
            r = super().gemm_nt_levels(lv, A, W, bias, a_packed, out_packed, pk)
            seen.append(tc._nt('gemm_nt_levels', lv.M, K, N, tc.BIAS if bias is not None else 0,
                               akind=tc.LEVELS if a_packed else tc.DENSE, ckind=tc.LEVELS if out_packed is not None else tc.DENSE,
                               pk=(0,) + tuple(pk), lv=(lv.B, tuple(lv.hw)), align=al(A, W, r, bias, None, None, None, None)))
            return r

        def gemm_tn_levels(self, lv, dY, X, N, K, y_packed=False, pk=(0, 0)):
            seen.append(tc._tn('gemm_tn_levels', lv.M, N, K, ykind=tc.LEVELS if y_packed else tc.DENSE, pk=(0,) + tuple(pk),
                               lv=(lv.B, tuple(lv.hw)), align=al(dY, X, None)))
            return super().gemm_tn_levels(lv, dY, X, N, K, y_packed, pk)

        def dw_fwd(self, x, taps, scale, shift, k, s):
            B, H, W, C = x.shape
            seen.append(('dw', 'fwd', B, H, W, C, k, s, int(bool(self.pad)), 0))
            return super().dw_fwd(x, taps, scale, shift, k, s)

        def dw_fwd_train(self, x, taps, scale, shift, k, s):
            B, H, W, C = x.shape
            seen.append(('dw', 'fwd', B, H, W, C, k, s, int(bool(self.pad)), 1))
            return super().dw_fwd_train(x, taps, scale, shift, k, s)

        def dw_bwd(self, dy, x, taps, k, s, z=None, out=None, cmajor=False):
            B, H, W, C = x.shape
            seen.append(('dw', 'bwd_dx', B, H, W, C, k, s, int(bool(self.pad)), int(z is not None)))
            seen.append(('dw', 'bwd_dw', B, H, W, C, k, s, int(bool(self.pad)), int(cmajor)))
            return super().dw_bwd(dy, x, taps, k, s, z=z, out=out, cmajor=cmajor)

    monkeypatch.setattr(te, '_Ops', Recording)
    size, B, C = 128, 2, 20
    assert B in tc.BATCHES and C in tc.NUM_CLASSES and size in tc.sizes_of('tf_efficientdet_d0')
    model, cfg, nodes, sd, x = _train_setup(size, B, C, seed=23)
    cls_t, box_t, npos = _targets(cfg, size, B, C, 6)
    model = model.to(DEV).float().train()
    model.backbone.apply(lambda m: m.eval() if isinstance(m, torch.nn.BatchNorm2d) else None)
    cls_o, box_o = model(x.to(DEV))
    total, _, _ = DetectionLoss(cfg)(cls_o, box_o, [t.to(DEV) for t in cls_t], [t.to(DEV) for t in box_t], npos.to(DEV))
    total.backward()
    torch.cuda.synchronize()
    assert isinstance(model._train_engine.ops, Recording)
    kinds = {(c[0], c[1]) for c in seen}
    assert kinds >= {('nt', 'gemm_nt'), ('nt', 'gemm_nt_fused'), ('nt', 'gemm_nt_levels'), ('tn', 'gemm_tn'), ('tn', 'gemm_tn_scaled'),
                     ('tn', 'gemm_tn_levels'), ('dw', 'fwd'), ('dw', 'bwd_dx'), ('dw', 'bwd_dw')}, kinds
    swept = {tc.call_class(lib, c) for c in tc.swept_calls('tf_efficientdet_d0', size, B)}
    recorded = {}
    for c in seen:
        recorded.setdefault(tc.call_class(lib, c), c)
    print('%d calls recorded, %d classes; the sweep has %d classes for this model, size and batch' % (len(seen), len(recorded), len(swept)))
    missing = {k: v for k, v in recorded.items() if k not in swept}
    assert not missing, missing
