#!/usr/bin/env python
"""csrc/logit_ood.hip without a GPU: the unit compiled by g++ against the CPU model of common.h (which models the float32-input
MFMA as the fmaf chain it is) and driven through its C ABI on numpy arrays - score and fit at C in {1, 7, 17, 90}, 1 .. 65 rows,
T in {1, 2.5} - against the restatement of tests/_logit_ood_ref.py.  It checks arithmetic, indexing and bounds (a guard region
follows every buffer), not timing or the memory model.

    python3 tools/simt_model/run_logit_ood.py [C T top_m]    needs g++ with C++20 (std::barrier); a thread per lane: about five minutes"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _logit_ood_ref as R  # noqa: E402
from _model import GUARD, build, guarded, ptr  # noqa: E402
from ood_object_detection_amd.ood_logits import finalize  # noqa: E402

FILL = -12345.5


class Model:
    """The device calls of ood_logits.LogitOOD on host memory"""

    def __init__(self, lib, C, T=1.0, gamma=0.1, top_m=10):
        self.lib, self.C, self.T, self.gamma, self.top_m = lib, C, T, gamma, top_m
        self.n_c, self._n = guarded((C,), np.int64, -7)
        self.P_c, self._P = guarded((C, C), np.float64, -7.5)
        self.a_c, self._a = guarded((C,), np.float64, -7.5)
        self.b_c, self._b = guarded((C,), np.float64, -7.5)
        for t in (self.n_c, self.P_c, self.a_c, self.b_c):
            t[...] = 0
        self.q = self.dev = None

    def head(self, z):
        es = z.itemsize
        B, N, C = z.shape
        assert C == 1 or z.strides[2] == es
        return (0 if es == 4 else 1, ptr(z), z.strides[0] // es, z.strides[1] // es, C, B, N)

    def fit(self, **kw):
        p = finalize(self.n_c, self.P_c, self.a_c, self.b_c, **kw)
        self.q = R.params(p)
        C, Cp = self.C, (self.C + 15) // 16 * 16
        log_d, self._ld = guarded((Cp, Cp), np.float32, 0)
        kl_inf, self._ki = guarded((Cp,), np.float32, np.inf)
        mu, self._mu = guarded((C,), np.float32, 0)
        isg, self._is = guarded((C,), np.float32, 0)
        self._ld[Cp * Cp:] = self._ki[Cp:] = self._mu[C:] = self._is[C:] = np.nan        # a read beyond a parameter poisons the row
        log_d[:C, :C], kl_inf[:C], mu[:], isg[:] = self.q['log_d'], self.q['kl_inf'], self.q['mu'], self.q['inv_sigma']
        self.dev = (log_d, kl_inf, mu, isg)

    def score(self, z, anchor=None, count=None):
        B, N, C = z.shape
        K = anchor.shape[1] if anchor is not None else N
        outs = {k: guarded((B, K), np.int64 if k.endswith('class') else np.float32, -99 if k.endswith('class') else FILL) for k in R.KEYS}
        fitted = [None] * 4 if self.dev is None else [ptr(t) for t in self.dev]
        o = lambda k: None if (self.dev is None and k in R.FITTED_KEYS) else ptr(outs[k][0])
        rc = self.lib.effdet_logit_ood_score(None, *self.head(z), K, ptr(anchor), ptr(count), int(count is not None and count.dtype == np.int64),
                                             self.T, self.gamma, self.top_m, *fitted, o('msp'), o('neg_entropy'), o('gen'), o('joint_energy'),
                                             o('predicted_class'), o('kl_matching'), o('kl_class'), o('standardized_max_logit'))
        assert rc == 0, rc
        for k, (v, w) in outs.items():
            assert (w[B * K:] == (-99 if k.endswith('class') else FILL)).all(), 'a write beyond an output: ' + k
            if self.dev is None and k in R.FITTED_KEYS:
                assert (v == (-99 if k.endswith('class') else FILL)).all(), 'a fitted key written without a fit'
        return {k: v for k, (v, w) in outs.items() if not (self.dev is None and k in R.FITTED_KEYS)}

    def add(self, z, anchor=None, count=None, min_max=None):
        B, N, C = z.shape
        K = anchor.shape[1] if anchor is not None else N
        nbytes = self.lib.effdet_logit_ood_workspace_bytes(B * K, C)
        assert nbytes > 0
        ws = np.full(nbytes + GUARD, 0xA5, np.uint8)
        args = (None, *self.head(z), K, ptr(anchor), ptr(count), int(count is not None and count.dtype == np.int64), self.T,
                int(min_max is not None), float(min_max or 0.0), ptr(self.n_c), ptr(self.P_c), ptr(self.a_c), ptr(self.b_c), ptr(ws))
        rc = self.lib.effdet_logit_ood_fit(*args, nbytes)
        assert rc == 0, rc
        assert (ws[nbytes:] == 0xA5).all(), 'a write beyond the workspace'
        C_ = self.C
        assert (self._n[C_:] == -7).all() and (self._P[C_ * C_:] == -7.5).all() and (self._a[C_:] == -7.5).all() and (self._b[C_:] == -7.5).all()
        assert self.lib.effdet_logit_ood_fit(*args, nbytes - 256) == -22


def place(z, B, rs):
    """n rows -> logits [B, N, C] with them at shuffled anchors, anchor [B, K], count [B] (the last image holds the remainder)"""
    n, C = z.shape
    K = -(-n // B)
    N = K + 5
    wide = rs.normal(size=(B + 1, N, C + 3)).astype(np.float32)
    lg = wide[:B, :, :C]                                                 # strided images and anchors, class stride 1
    anchor = np.stack([rs.permutation(N)[:K] for _ in range(B)]).astype(np.int64)
    count = np.clip(n - K * np.arange(B), 0, K).astype(np.int32)
    zs = np.zeros((B * K, C), np.float32)
    zs[:n] = z
    live = np.arange(K)[None, :] < count[:, None]
    lg[np.arange(B)[:, None].repeat(K, 1)[live], anchor[live]] = zs.reshape(B, K, C)[live]
    return lg, anchor, count, live


def bits_eq(a, b):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a) and set(a) == set(b)


def run(lib, C, T, top_m):
    d = R.inputs(C, 300, 65)
    rs = np.random.RandomState(C + top_m)
    m = Model(lib, C, T, 0.1, top_m)
    # fit: the 300 rows in two calls, the second one dense with a threshold; n_c exact, the sums against numpy
    lg, anchor, count, live = place(d['z_fit'][:200], 3, rs)
    m.add(lg, anchor, count)
    dense = np.ascontiguousarray(d['z_fit'][200:].reshape(2, 50, C))
    thr = float(np.median(d['z_fit'][200:].max(1)))
    m.add(dense, min_max=thr)
    kept = np.concatenate([d['z_fit'][:200], d['z_fit'][200:][d['z_fit'][200:].max(1) >= np.float32(thr)]])
    n_c, P_c, a_c, b_c = R.stats(kept, C, T)
    assert np.array_equal(m.n_c, n_c), (m.n_c, n_c)
    mz = kept.max(1).astype(np.float64)
    assert np.abs(m.a_c - a_c).max() <= len(kept) * 2.0 ** -50 * np.abs(mz).sum()
    assert np.abs(m.b_c - b_c).max() <= len(kept) * 2.0 ** -50 * (mz * mz).sum()
    p32 = np.abs(R.softmax(kept, 1.0, np.float32)['p'].astype(np.float64) - R.softmax(kept, 1.0)['p']).max()
    assert np.abs(m.P_c - P_c).max() <= max(n_c.max(), 1) * (4 * p32 + 1e-7), (np.abs(m.P_c - P_c).max(), p32)
    # the indexed form of the dense rows gives the same bits
    m2 = Model(lib, C, T, 0.1, top_m)
    m2.add(lg, anchor, count)
    m2.add(dense, np.tile(np.arange(50, dtype=np.int64), (2, 1)), None, min_max=thr)
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in ((m.n_c, m2.n_c), (m.P_c, m2.P_c), (m.a_c, m2.a_c), (m.b_c, m2.b_c)))
    # before the fit: five keys
    z = np.concatenate([d['z_in'][:33], d['z_ood'][:32]])
    unfit = m.score(np.ascontiguousarray(z[None]))
    assert set(unfit) == set(R.KEYS) - set(R.FITTED_KEYS)
    m.fit()
    kw = dict(T=T, gamma=0.1, top_m=top_m, q=m.q)
    full, f32 = R.score(z, **kw), R.score(z, np.float32, **kw)
    bnd = R.bounds(full, f32)
    worst = {k: 0.0 for k in R.FLOAT_KEYS}
    for n, B in ((1, 1), (15, 1), (16, 1), (17, 2), (63, 1), (64, 2), (65, 3)):
        lg, anchor, count, live = place(z[:n], B, rs)
        got = m.score(lg, anchor, count)
        for k in R.FLOAT_KEYS:
            err = np.abs(got[k][live] - full[k][:n]).max()
            assert err <= bnd[k][1], (C, T, n, k, err, bnd[k])
            assert (got[k][~live] == 0).all(), (C, n, k)
            worst[k] = max(worst[k], err / bnd[k][1] if bnd[k][1] else 0.0)
        assert np.array_equal(got['predicted_class'][live], full['predicted_class'][:n]) and (got['predicted_class'][~live] == -1).all()
        sure = full['kl_margin'][:n] >= 2 * bnd['kl_matching'][1]
        assert np.array_equal(got['kl_class'][live][sure], full['kl_class'][:n][sure]) and (got['kl_class'][~live] == -1).all()
        # packed logits, int64 counts -> bitwise; every anchor against the identity index -> bitwise; and against the indexed rows
        packed = np.ascontiguousarray(lg)
        assert bits_eq(m.score(packed, anchor, count.astype(np.int64)), got)
        dense_s = m.score(lg)
        assert bits_eq(m.score(packed, np.tile(np.arange(lg.shape[1], dtype=np.int64), (B, 1))), dense_s)
        for k in got:
            assert np.array_equal(np.take_along_axis(dense_s[k], anchor, 1)[live].view(np.uint8), got[k][live].view(np.uint8)), k
        # bfloat16 logits against their float32 widening -> bitwise
        bits = (packed.view(np.uint32) >> 16).astype(np.uint16)
        assert bits_eq(m.score(bits, anchor, count), m.score(R.widen_bf16(bits), anchor, count))
    # exact ties: the lowest index is the predicted class, and the top_m boundary takes the lower classes first
    t = np.full((1, 1, C), -2.0, np.float32)
    if C >= 3:
        t[0, 0, [1, 2]] = 3.0
        t[0, 0, 0] = 1.0
    got, ref = m.score(t), R.score(t[0], **kw)
    tb = R.bounds(ref, R.score(t[0], np.float32, **kw))['gen'][1]                   # this row's own float32 error
    assert got['predicted_class'][0, 0] == ref['predicted_class'][0] == (1 if C >= 3 else 0)
    assert abs(got['gen'][0, 0] - ref['gen'][0]) <= max(tb, bnd['gen'][1]), (got['gen'][0, 0], ref['gen'][0], tb)
    # +88 and -100 in one row stay finite; a NaN row spoils nothing but itself
    ext = np.ascontiguousarray(z[:16][None]).copy()
    ext[0, 3, :] = -100.0
    ext[0, 3, 0] = 88.0
    a = m.score(ext)
    assert all(np.isfinite(a[k][0, 3]) for k in R.FLOAT_KEYS), {k: a[k][0, 3] for k in R.FLOAT_KEYS}
    ext2 = ext.copy()
    ext2[0, 5, C // 2] = np.nan
    b = m.score(ext2)
    keep = np.arange(16) != 5
    assert all(np.array_equal(a[k][0, keep].view(np.uint8), b[k][0, keep].view(np.uint8)) for k in a)
    print('C %4d, T %.1f, top_m %3d: fit and score ok; worst error / bound: %s' % (C, T, top_m, ', '.join('%s %.2f' % kv for kv in worst.items())))


def refusals(lib):
    z = np.zeros((1, 4, 7), np.float32)
    out = np.zeros((1, 4), np.float32)
    cls = np.zeros((1, 4), np.int64)
    par = np.zeros((16, 16), np.float32)

    def call(C=7, B=1, N=4, K=4, T=1.0, gamma=0.1, top_m=10, bs=28, as_=7, fitted=(None,) * 4, kl=(None,) * 3, msp=ptr(out)):
        return lib.effdet_logit_ood_score(None, 0, ptr(z), bs, as_, C, B, N, K, None, None, 0, T, gamma, top_m, *fitted, msp, ptr(out), ptr(out),
                                          ptr(out), ptr(cls), *kl)
    assert call() == 0
    full = (ptr(par),) * 4
    for kw in (dict(C=0), dict(C=1025), dict(B=0), dict(N=0), dict(K=0), dict(T=0.0), dict(T=-1.0), dict(T=float('nan')), dict(top_m=0),
               dict(gamma=float('inf')), dict(bs=-1), dict(as_=-1), dict(msp=None), dict(fitted=full), dict(kl=(ptr(out), ptr(cls), ptr(out))),
               dict(B=1 << 14, K=1 << 14)):
        assert call(**kw) == -22, kw
    q = lib.effdet_logit_ood_workspace_bytes
    assert q(0, 7) == -22 and q((1 << 27) + 1, 7) == -22 and q(4, 0) == -22 and q(4, 1025) == -22 and 0 < q(1, 1) <= q(100, 90)
    print('refusals ok')


def main():
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(tmp, 'logit_ood', 'effdet_logit_ood_')
        refusals(lib)
        if len(sys.argv) == 4:                                   # one case of the caller's: C T top_m
            run(lib, int(sys.argv[1]), float(sys.argv[2]), int(sys.argv[3]))
            return
        for C, T, top_m in ((1, 1.0, 10), (7, 1.0, 1), (7, 2.5, 10), (17, 1.0, 10), (17, 2.5, 22), (90, 1.0, 10), (90, 2.5, 1)):
            run(lib, C, T, top_m)
    print('logit_ood on the CPU model: all checks passed')


if __name__ == '__main__':
    main()
