#!/usr/bin/env python
"""csrc/feature_ood.hip without a GPU: the unit compiled by g++ against the CPU model of common.h (which models the float32-input
MFMA as the fmaf chain it is) and driven through its C ABI on numpy arrays - the fit (compaction, scatter-matrix partials, class
sums) and the score at small shapes of tests/test_feature_ood_gpu.py - against the restatement of tests/_feature_ood_ref.py.  It
checks arithmetic, indexing and bounds (a guard region follows every buffer), not timing or the memory model.

    python3 tools/simt_model/run_feature_ood.py [--wide]    needs g++ with C++20 (std::barrier); a thread per lane, so minutes
                                                            (--wide: also F = 288, several minutes more)"""
import ctypes
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _feature_ood_ref as R  # noqa: E402
from _model import GUARD, build, guarded, ptr  # noqa: E402


def lls(v):
    return (ctypes.c_longlong * len(v))(*[int(x) for x in v])


class Model:
    """The calls of ood_features.FeatureOOD on host memory; levels: list of [B, cells, F] float32 arrays (any strides with a unit
    channel stride) or uint16 arrays holding bfloat16 bits"""

    def __init__(self, lib, F, C, A):
        self.lib, self.F, self.C, self.A = lib, F, C, A
        self.n_c, self._n = guarded((C,), np.int64, -7)
        self.s_c, self._s = guarded((C, F), np.float64, -7.5)
        self.S, self._S = guarded((F, F), np.float64, -7.5)
        self.n_c[:] = 0
        self.s_c[:] = 0
        self.S[:] = 0

    def table(self, levels):
        es = levels[0].itemsize
        return (0 if es == 4 else 1, len(levels), (ctypes.c_void_p * len(levels))(*[l.ctypes.data for l in levels]),
                lls([l.shape[1] for l in levels]), lls([l.strides[0] // es for l in levels]), lls([l.strides[1] // es for l in levels]),
                lls([l.strides[2] // es for l in levels]))

    def add(self, levels, classes, anchor=None, count=None, offset=0):
        B, K = classes.shape
        rows = B * K
        nbytes = self.lib.effdet_feature_ood_workspace_bytes(rows, self.F)
        assert nbytes > 0
        ws = np.full(nbytes + GUARD, 0xA5, np.uint8)
        cdt = {np.dtype(np.int32): 0, np.dtype(np.int64): 1, np.dtype(np.float32): 2}[classes.dtype]
        es = classes.itemsize
        rc = self.lib.effdet_feature_ood_fit(None, *self.table(levels), self.F, self.C, self.A, B, K, ptr(anchor), ptr(classes), cdt,
                                             classes.strides[0] // es, classes.strides[1] // es, offset, ptr(count),
                                             int(count is not None and count.dtype == np.int64), ptr(self.n_c), ptr(self.s_c), ptr(self.S),
                                             ptr(ws), nbytes)
        assert rc == 0, rc
        assert (ws[nbytes:] == 0xA5).all(), 'a write beyond the workspace'
        assert (self._n[self.C:] == -7).all() and (self._s[self.C * self.F:] == -7.5).all() and (self._S[self.F * self.F:] == -7.5).all(), \
            'a write beyond a statistics buffer'

    def score(self, levels, p, anchor=None, count=None, A=None):
        F, C = self.F, self.C
        Fp, Cp = (F + 15) // 16 * 16, (C + 31) // 32 * 32
        W, W0, M = np.zeros((Fp, Fp), np.float32), np.zeros((Fp, Fp), np.float32), np.zeros((Cp, Fp), np.float32)
        m2, mu0 = np.full(Cp, np.inf, np.float32), np.zeros(Fp, np.float32)
        W[:F, :F], W0[:F, :F], M[:C, :F], m2[:C], mu0[:F] = p['W'], p['W0'], p['M'], p['m2'], p['mu0']
        B = levels[0].shape[0]
        A = self.A if A is None else A
        K = anchor.shape[1] if anchor is not None else A * sum(l.shape[1] for l in levels)
        maha, _m = guarded((B, K), np.float32, -12345.5)
        rel, _r = guarded((B, K), np.float32, -12345.5)
        near, _k = guarded((B, K), np.int32, -777)
        rc = self.lib.effdet_feature_ood_score(None, *self.table(levels), F, C, A, B, K, ptr(anchor), ptr(count),
                                               int(count is not None and count.dtype == np.int64), ptr(W), ptr(W0), ptr(M), ptr(m2), ptr(mu0),
                                               ptr(maha), ptr(rel), ptr(near))
        assert rc == 0, rc
        assert (_m[B * K:] == -12345.5).all() and (_r[B * K:] == -12345.5).all() and (_k[B * K:] == -777).all(), 'a write beyond an output'
        return maha, rel, near


def check_fit(m, x, y, name):
    n_c, s_c, S = R.fit(x, y, m.C)
    assert np.array_equal(m.n_c, n_c), name
    for got, ref, what in ((m.s_c, s_c, 's_c'), (m.S, S, 'S')):
        err = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300)
        assert err <= 1e-12, (name, what, err)
    assert np.array_equal(m.S, m.S.T), name
    print('%-44s fit ok: %d rows' % (name, int(n_c.sum())))


def run(lib, F, C, n_fit=300, n_score=70):
    A = 3
    d = R.inputs(F, C, n_fit, n_score)
    rs = np.random.RandomState(F + C)
    # a two-level pyramid [B, P, F] with cells scattered over it; anchors a * cell + (0 .. A - 1)
    B, cells = 3, (max(150, n_fit // 3), 37)
    P = sum(cells)
    pyr = rs.normal(size=(B, P, F)).astype(np.float32)
    K = n_fit // B
    cell = np.stack([rs.permutation(P)[:K] for _ in range(B)])
    pyr[np.arange(B)[:, None], cell] = d['x_fit'][:B * K].reshape(B, K, F)
    anchor = (cell * A + rs.randint(0, A, cell.shape)).astype(np.int64)
    y = d['y_fit'][:B * K].reshape(B, K).copy()
    y[0, 3], y[1, 5] = -1, C                                          # skipped: ignore label, class >= C
    count = np.array([K, K - 7, 1], np.int32)
    valid = (np.arange(K)[None, :] < count[:, None]) & (y >= 0) & (y < C)
    levels = [pyr[:, :cells[0]], pyr[:, cells[0]:]]                  # views of one buffer
    m = Model(lib, F, C, A)
    m.add(levels, y, anchor, count)
    check_fit(m, pyr[np.arange(B)[:, None], cell][valid], y[valid], 'F %d C %d: indexed, two levels, int64' % (F, C))
    first = (m.n_c.copy(), m.s_c.copy(), m.S.copy())
    # the same rows: one level, float32 classes with an offset, int64 counts -> bitwise
    m2 = Model(lib, F, C, A)
    m2.add([pyr], (y + 1).astype(np.float32), anchor, count.astype(np.int64), offset=1)
    assert all(np.array_equal(a, b) for a, b in zip(first, (m2.n_c, m2.s_c, m2.S))), 'one level against two'
    # the dense form: labels [B, A * P], -1 everywhere but on the chosen anchors
    dense = np.full((B, A * P), -1, np.int32)
    for b in range(B):
        dense[b, anchor[b][valid[b]]] = y[b][valid[b]]
    m3 = Model(lib, F, C, A)
    m3.add(levels, dense)
    order = np.argsort(anchor, 1)                                     # the dense scan visits the anchors in ascending order
    m4 = Model(lib, F, C, A)
    m4.add(levels, np.take_along_axis(np.where(valid, y, -1), order, 1), np.take_along_axis(anchor, order, 1))
    assert all(np.array_equal(a, b) for a, b in zip((m3.n_c, m3.s_c, m3.S), (m4.n_c, m4.s_c, m4.S))), 'dense against indexed'
    assert np.array_equal(m3.n_c, first[0])
    # bfloat16 features against their float32 widening -> bitwise
    bits = (pyr.view(np.uint32) >> 16).astype(np.uint16)
    wide = (bits.astype(np.uint32) << 16).view(np.float32)
    m5, m6 = Model(lib, F, C, A), Model(lib, F, C, A)
    m5.add([bits], y, anchor, count)
    m6.add([wide], y, anchor, count)
    assert all(np.array_equal(a, b) for a, b in zip((m5.n_c, m5.s_c, m5.S), (m6.n_c, m6.s_c, m6.S))), 'bfloat16 against its widening'
    print('%-44s one level, dense form, bfloat16: bitwise ok' % '')

    # score: parameters from the whole fit set; rows placed in the pyramid, some beyond count
    p = R.finalize(*R.fit(d['x_fit'], d['y_fit'], C))
    if C > 2:
        p['m2'] = p['m2'].copy(); p['m2'][1] = np.inf; p['have'] = p['have'].copy(); p['have'][1] = False       # an empty class never wins
    Ks = n_score // B
    xs = d['x_ood'][:B * Ks].reshape(B, Ks, F)
    cell = np.stack([rs.permutation(P)[:Ks] for _ in range(B)])
    pyr[np.arange(B)[:, None], cell] = xs
    anchor = (cell * A + rs.randint(0, A, cell.shape)).astype(np.int64)
    count = np.array([Ks, Ks - 5, 0], np.int32)
    live = np.arange(Ks)[None, :] < count[:, None]
    maha, rel, near = m.score(levels, p, anchor, count)
    ref, f32 = R.score(xs.reshape(-1, F), p), R.score(xs.reshape(-1, F), p, np.float32)
    e32, bound = R.score_bound(ref, f32)
    lv = live.reshape(-1)
    err = max(np.abs(maha.reshape(-1)[lv] - ref['mahalanobis'][lv]).max(), np.abs(rel.reshape(-1)[lv] - ref['relative'][lv]).max())
    assert err <= bound, (err, bound)
    assert np.array_equal(near.reshape(-1)[lv], ref['nearest'][lv]) and not R.near_ties(ref, bound).any()
    assert (maha[~live] == 0).all() and (rel[~live] == 0).all() and (near[~live] == -1).all()
    if C > 2:
        assert not (near == 1).any()
    # every cell, against the indexed form with the identity index and A = 1 -> bitwise
    c_m, c_r, c_n = m.score(levels, p, A=1)
    ident = np.tile(np.arange(P, dtype=np.int64), (B, 1))
    i_m, i_r, i_n = m.score([pyr], p, ident, A=1)
    assert np.array_equal(c_m.view(np.uint32), i_m.view(np.uint32)) and np.array_equal(c_r.view(np.uint32), i_r.view(np.uint32)) and np.array_equal(c_n, i_n)
    assert np.array_equal(c_m[np.arange(B)[:, None], cell][live].view(np.uint32), maha[live].view(np.uint32))
    print('%-44s score ok: error %.2e, E32 %.2e, bound %.2e' % ('F %d C %d' % (F, C), err, e32, bound))


def main():
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(tmp, 'feature_ood', 'effdet_feature_ood_')
        run(lib, 64, 1)
        run(lib, 88, 7)
        run(lib, 64, 90, n_fit=600)
        if '--wide' in sys.argv[1:]:
            run(lib, 288, 33, n_fit=900)


if __name__ == '__main__':
    main()
