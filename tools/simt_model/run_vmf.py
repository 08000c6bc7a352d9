#!/usr/bin/env python
"""csrc/vmf.hip without a GPU: the unit compiled by g++ against the CPU model of common.h and driven through its C ABI on numpy
arrays - the partition function on a grid of (d, kappa), the ordered prototype update (bit for bit against the float32 restatement),
the loss with dU, d theta and the statistics, the scores and the gather - against the restatement of tests/_vmf_ref.py.  It checks
arithmetic, indexing and bounds (a guard region follows every buffer), not timing or the memory model.

    python3 tools/simt_model/run_vmf.py    needs g++ with C++20 (std::barrier); a thread per lane: a few minutes"""
import ctypes
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _vmf_ref as R  # noqa: E402
from _model import GUARD, build, guarded, ptr  # noqa: E402

FILL = -12345.5
REL = 2.0 ** -30


def workspace(lib, rows, C, d):
    n = lib.effdet_vmf_workspace_bytes(rows, C, d)
    assert n > 0, n
    return np.full(n + GUARD, 0xA5, np.uint8), n


def partition(lib, theta, d):
    C = len(theta)
    th = np.ascontiguousarray(theta, np.float32)
    kappa, _k = guarded((C,), np.float32, FILL)
    lz, _l = guarded((C,), np.float32, FILL)
    lz64, _m = guarded((C,), np.float64, FILL)
    ratio, _r = guarded((C,), np.float64, FILL)
    cl, _c = guarded((C,), np.int32, 77)
    assert lib.effdet_vmf_partition(None, ptr(th), C, d, ptr(kappa), ptr(lz), ptr(lz64), ptr(ratio), ptr(cl)) == 0
    assert (_k[C:] == FILL).all() and (_l[C:] == FILL).all() and (_m[C:] == FILL).all() and (_r[C:] == FILL).all() and (_c[C:] == 77).all()
    return {'kappa': kappa.copy(), 'logz32': lz.copy(), 'logz': lz64.copy(), 'ratio': ratio.copy(), 'clamped': cl.astype(bool)}


def class_args(labels):
    code = {np.dtype(np.int32): 0, np.dtype(np.int64): 1, np.dtype(np.float32): 2}[labels.dtype]
    return ptr(labels), code, labels.shape[1], 1, 0


def update(lib, U, labels, A, proto, valid, alpha, limit):
    B, P, d = U.shape
    C = proto.shape[0]
    pr, _p = guarded((C, d), np.float32, FILL)
    pr[:] = proto
    va, _v = guarded((C,), np.int32, 77)
    va[:] = valid
    ws, n = workspace(lib, B * A * P, C, d)
    args = (None, ptr(U), B, P, A, d, *class_args(labels), C, alpha, limit or 0, ptr(pr), ptr(va), ptr(ws))
    assert lib.effdet_vmf_update(*args, n) == 0
    assert (ws[n:] == 0xA5).all(), 'a write beyond the workspace'
    assert (_p[C * d:] == FILL).all() and (_v[C:] == 77).all(), 'a write beyond an output'
    assert lib.effdet_vmf_update(*args, n - 256) == -22
    return pr.copy(), va.astype(bool)


def loss(lib, U, labels, A, proto, valid, part):
    B, P, d = U.shape
    C = proto.shape[0]
    lo, _l = guarded((1,), np.float32, FILL)
    st, _s = guarded((8,), np.float64, FILL)
    dU, _u = guarded((B, P, d), np.float32, FILL)
    dth, _t = guarded((C,), np.float32, FILL)
    ws, n = workspace(lib, B * A * P, C, d)
    pr, va = np.ascontiguousarray(proto, np.float32), np.ascontiguousarray(valid, np.int32)
    cl = np.ascontiguousarray(part['clamped'], np.int32)
    args = (None, ptr(U), B, P, A, d, *class_args(labels), C, ptr(pr), ptr(va), ptr(part['kappa']), ptr(part['logz32']), ptr(part['ratio']),
            ptr(cl), ptr(lo), ptr(st), ptr(dU), ptr(dth), ptr(ws))
    assert lib.effdet_vmf_loss(*args, n) == 0
    assert (ws[n:] == 0xA5).all(), 'a write beyond the workspace'
    assert (_l[1:] == FILL).all() and (_s[8:] == FILL).all() and (_u[B * P * d:] == FILL).all() and (_t[C:] == FILL).all(), 'a write beyond an output'
    assert lib.effdet_vmf_loss(*args, n - 256) == -22
    return {'loss': lo[0], 'stats': st.copy(), 'dU': dU.copy(), 'dtheta': dth.copy()}


def score(lib, U, A, proto, valid, part, anchor=None, count=None, gathered=False, K=None):
    B, P, d = U.shape
    C = proto.shape[0]
    if gathered:
        K, Pn = P, K                                             # U is [B, K, d]; Pn: the cells the anchors index
    else:
        K, Pn = (anchor.shape[1] if anchor is not None else A * P), P
    v, _v = guarded((B, K), np.float32, FILL)
    c, _c = guarded((B, K), np.int64, 77)
    s, _s = guarded((B, K), np.float32, FILL)
    rw, _r = guarded((B, K, d), np.float32, FILL)
    ws, n = workspace(lib, B * K, C, d)
    pr, va = np.ascontiguousarray(proto, np.float32), np.ascontiguousarray(valid, np.int32)
    rc = lib.effdet_vmf_score(None, ptr(U), B, Pn, A, d, K, ptr(anchor), ptr(count), int(count is not None and count.dtype == np.int64),
                              int(gathered), C, ptr(pr), ptr(va), ptr(part['kappa']), ptr(part['logz32']), ptr(v), ptr(c), ptr(s), ptr(rw),
                              ptr(ws), n)
    assert rc == 0, rc
    assert (ws[n:] == 0xA5).all() and (_v[B * K:] == FILL).all() and (_c[B * K:] == 77).all() and (_s[B * K:] == FILL).all()
    assert (_r[B * K * d:] == FILL).all()
    return {'vmf': v.copy(), 'vmf_class': c.copy(), 'vmf_cosine': s.copy(), 'rows': rw.copy()}


def check_partition(lib):
    worst = [0.0, 0.0]
    for d in (2, 3, 4, 16, 17, 64, 255, 256):
        kap = np.array([2.0 ** -7, 0.3, 1, 10, 100, 1000, 8192], np.float64)
        theta = np.log(kap).astype(np.float32)
        got, ref = partition(lib, theta, d), R.partition(theta, d)
        assert np.abs(got['kappa'].view(np.int32) - ref['kappa'].view(np.int32)).max() <= 1 and not got['clamped'].any(), d
        at = R.from_kappa(got['kappa'], d)                       # the table at the device's own concentrations
        e1 = np.abs(got['logz'] - at['logz']) / np.maximum(1.0, np.abs(at['logz']))
        e2 = np.abs(got['ratio'] - at['ratio']) / at['ratio']
        assert e1.max() <= REL and e2.max() <= REL, (d, e1.max(), e2.max())
        assert np.array_equal(got['logz32'], got['logz'].astype(np.float32))
        worst = [max(worst[0], e1.max()), max(worst[1], e2.max())]
    out = partition(lib, np.array([-100.0, 100.0, np.nan, R.THETA_LO, R.THETA_HI], np.float32), 64)
    assert list(out['clamped']) == [True, True, True, False, False]
    assert np.abs(out['kappa'] / np.array([2.0 ** -7, 8192, 2.0 ** -7, 2.0 ** -7, 8192]) - 1).max() <= 1e-6      # (the ends of the clamp are float32 logarithms)
    print('partition: ok; worst relative error logZ %.1e, ratio %.1e' % tuple(worst))


def check_case(lib, B, P, d, A, C, n, limit=None, nan_row=False):
    U, labels = R.inputs(B, P, d, A, C, n)
    if nan_row:
        U[0, 0, d // 2], labels[0, 0] = np.nan, 0               # a counted anchor on a row that holds a NaN: skipped
    name = 'B %d P %d d %d A %d C %d counted %d limit %r' % (B, P, d, A, C, n, limit)
    proto0, valid0 = np.zeros((C, d), np.float32), np.zeros(C, bool)
    pr, va = update(lib, U, labels, A, proto0, valid0, 0.95, limit)
    pr_ref, va_ref = R.update(U, labels, A, proto0, valid0, 0.95, limit)
    assert np.array_equal(pr.view(np.uint32), pr_ref.view(np.uint32)) and np.array_equal(va, va_ref), name
    theta = np.log(np.random.RandomState(C).uniform(2.0, 40.0, C)).astype(np.float32)
    if C > 2:
        theta[1] = 20.0                                          # beyond the clamp: no gradient
    part = partition(lib, theta, d)
    got = loss(lib, U, labels.astype(np.int32) if C % 2 else labels, A, pr, va, part)
    ref, f32 = R.forward(U, labels, A, pr, va, part), R.forward(U, labels, A, pr, va, part, np.float32)
    bnd = R.bounds(ref, f32)
    worst = 0.0
    for k, dev in (('loss', got['loss']), ('dU', got['dU']), ('dtheta', got['dtheta']), ('mean_dot', got['stats'][3])):
        err = float(np.abs(np.asarray(dev, np.float64) - ref[k]).max())
        assert err <= bnd[k][1], (name, k, err, bnd[k])
        worst = max(worst, err / bnd[k][1] if bnd[k][1] else 0.0)
    assert [int(v) for v in got['stats'][:3]] == [ref['m'], ref['skipped'], ref['valid_classes']], (name, got['stats'])
    assert abs(got['stats'][4] - ref['mean_kappa']) <= 1e-12 * ref['mean_kappa'] and got['stats'][5] == ref['max_kappa']
    if C > 2:
        assert got['dtheta'][1] == 0
    counted = np.zeros(B * P, bool)
    counted[ref['idx'] // A] = True
    assert not got['dU'].reshape(B * P, d)[~counted].any(), name
    # scores: every cell, then selected anchors of the dense tensor and of a gathered copy, bit for bit
    cells = score(lib, U, 1, pr, va, part)
    rs = R.score(U.reshape(B * P, d), pr, va, part)
    f = R.score(U.reshape(B * P, d), pr, va, part, np.float32)
    fin = np.isfinite(U).all(2).reshape(-1)
    for k in ('vmf', 'vmf_cosine'):
        e32, bd = R.bound(rs[k][fin], f[k][fin])
        assert np.abs(cells[k].reshape(-1)[fin] - rs[k][fin]).max() <= bd, (name, k)
    sure = fin & (rs['margin'] > 2 * R.bound(rs['vmf'][fin], f['vmf'][fin])[1])
    assert np.array_equal(cells['vmf_class'].reshape(-1)[sure], rs['vmf_class'][sure]), name
    assert (cells['vmf_class'].reshape(-1)[~fin] == -1).all() and np.isnan(cells['vmf'].reshape(-1)[~fin]).all()
    rr = np.random.RandomState(5)
    Ksel = 11
    anchor = rr.randint(0, A * P, (B, Ksel)).astype(np.int64)
    anchor[0, 3], anchor[B - 1, 5] = -1, A * P
    count = np.array([Ksel - 2] + [Ksel] * (B - 1), np.int32)
    sel = score(lib, U, A, pr, va, part, anchor, count)
    okm = (np.arange(Ksel)[None] < count[:, None]) & (anchor >= 0) & (anchor < A * P)
    cell = np.where(okm, anchor // A, 0)
    for k in ('vmf', 'vmf_class', 'vmf_cosine'):
        want = np.take_along_axis(cells[k], cell, 1)
        want = np.where(okm, want, -1 if k == 'vmf_class' else 0)
        assert np.array_equal(sel[k].view(np.uint8), want.astype(sel[k].dtype).view(np.uint8)), (name, k)
    gathered = np.ascontiguousarray(np.take_along_axis(U, cell[:, :, None], 1))
    g = score(lib, gathered, A, pr, va, part, anchor, count, gathered=True, K=P)
    assert all(np.array_equal(g[k].view(np.uint8), sel[k].view(np.uint8)) for k in g), name
    assert not sel['rows'][~okm].any()
    print('%s: ok; worst error / bound %.2f' % (name, worst))


def check_gather(lib):
    rs = np.random.RandomState(3)
    B, F, A = 2, 64, 3
    shapes = ((4, 4), (2, 2), (1, 1))
    levels = [rs.normal(size=(B, h, w, F)).astype(np.float32) for h, w in shapes]
    P = sum(h * w for h, w in shapes)
    K = 13
    anchor = rs.randint(0, A * P, (B, K)).astype(np.int64)
    anchor[1, 2] = A * P
    count = np.array([K, K - 3], np.int64)
    for bf16 in (False, True):
        lv = [(t.view(np.uint32) >> 16).astype(np.uint16) for t in levels] if bf16 else levels
        wide = [(t.astype(np.uint32) << 16).view(np.float32) for t in lv] if bf16 else levels
        out, _o = guarded((B * K, F), np.float32, FILL)
        arr = lambda v, t: (t * len(v))(*v)
        rc = lib.effdet_vmf_gather(None, int(bf16), len(lv), arr([t.ctypes.data for t in lv], ctypes.c_void_p),
                                   arr([h * w for h, w in shapes], ctypes.c_longlong), arr([h * w * F for h, w in shapes], ctypes.c_longlong),
                                   arr([F] * 3, ctypes.c_longlong), arr([1] * 3, ctypes.c_longlong), F, A, B, K, ptr(anchor), ptr(count), 1, ptr(out))
        assert rc == 0 and (_o[B * K * F:] == FILL).all()
        flat = np.concatenate([t.reshape(B, -1, F) for t in wide], 1)
        ok = (np.arange(K)[None] < count[:, None]) & (anchor < A * P)
        want = np.where(ok[:, :, None], np.take_along_axis(flat, np.where(ok, anchor // A, 0)[:, :, None], 1), 0).reshape(B * K, F)
        assert np.array_equal(out, want), bf16
    print('gather: ok')


def refusals(lib):
    U, lab = np.zeros((1, 4, 8), np.float32), np.zeros((1, 8), np.int64)
    f, dd, ii = np.zeros(64, np.float32), np.zeros(64, np.float64), np.zeros(64, np.int32)
    n = lib.effdet_vmf_workspace_bytes(8, 3, 8)
    ws = np.zeros(n, np.uint8)

    def up(U=ptr(U), B=1, P=4, A=2, d=8, cls=ptr(lab), dt=1, C=3, alpha=0.9, lim=0, pr=ptr(f), va=ptr(ii), w=ptr(ws), nb=n):
        return lib.effdet_vmf_update(None, U, B, P, A, d, cls, dt, 8, 1, 0, C, alpha, lim, pr, va, w, nb)
    assert up() == 0
    for kw in (dict(U=None), dict(B=0), dict(P=0), dict(A=0), dict(d=1), dict(d=257), dict(cls=None), dict(dt=3), dict(C=0), dict(C=1025),
               dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=float('nan')), dict(lim=-1), dict(pr=None), dict(va=None), dict(w=None), dict(nb=n - 1)):
        assert up(**kw) == -22, kw
    q = lib.effdet_vmf_workspace_bytes
    assert q(0, 3, 8) == -22 and q((1 << 27) + 1, 3, 8) == -22 and q(8, 0, 8) == -22 and q(8, 1025, 8) == -22 and q(8, 3, 1) == -22 and q(8, 3, 257) == -22
    assert lib.effdet_vmf_partition(None, None, 3, 8, ptr(f), ptr(f), ptr(dd), ptr(dd), ptr(ii)) == -22
    assert lib.effdet_vmf_partition(None, ptr(f), 3, 1, ptr(f), ptr(f), ptr(dd), ptr(dd), ptr(ii)) == -22
    print('refusals ok')


def main():
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(tmp, 'vmf', 'effdet_vmf')
        refusals(lib)
        check_partition(lib)
        check_gather(lib)
        check_case(lib, 1, 9, 2, 1, 1, 5)
        check_case(lib, 2, 20, 16, 3, 7, 40)
        check_case(lib, 2, 20, 16, 3, 7, 40, limit=2, nan_row=True)
        check_case(lib, 2, 12, 65, 2, 65, 30)
        check_case(lib, 2, 8, 256, 1, 130, 12)
        check_case(lib, 1, 1100, 8, 2, 3, 2100)
        check_case(lib, 2, 6, 4, 9, 4, 0)
    print('vmf on the CPU model: all checks passed')


if __name__ == '__main__':
    main()
