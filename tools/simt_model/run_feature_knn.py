#!/usr/bin/env python
"""csrc/feature_knn.hip without a GPU: the unit compiled by g++ against the CPU model of common.h (which models the float32-input
MFMA as the fmaf chain it is) and driven through its C ABI on numpy arrays - append (compaction, sampling, overflow) and score
(bank walk, per-lane lists, merge) at the smallest shapes of tests/test_feature_knn_gpu.py - against the restatement of
tests/_feature_knn_ref.py.  It checks arithmetic, indexing and bounds (a guard region follows every buffer), not timing or the
memory model.

    python3 tools/simt_model/run_feature_knn.py     needs g++ with C++20 (std::barrier); a thread per lane, so minutes"""
import ctypes
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _feature_knn_ref as R  # noqa: E402
from _model import GUARD, build, guarded, ptr  # noqa: E402


def lls(v):
    return (ctypes.c_longlong * len(v))(*[int(x) for x in v])


def table(levels):
    es = levels[0].itemsize
    return (0 if es == 4 else 1, len(levels), (ctypes.c_void_p * len(levels))(*[l.ctypes.data for l in levels]),
            lls([l.shape[1] for l in levels]), lls([l.strides[0] // es for l in levels]), lls([l.strides[1] // es for l in levels]),
            lls([l.strides[2] // es for l in levels]))


class Model:
    """The calls of ood_features.KNNFeatureOOD on host memory; levels: list of [B, cells, F] float32 arrays"""

    def __init__(self, lib, F, A, capacity, C=0, normalize=True, every=1):
        self.lib, self.F, self.A, self.cap, self.C, self.normalize, self.every = lib, F, A, capacity, C, normalize, every
        self.Fp = (F + 15) // 16 * 16
        self.bank, self._b = guarded((capacity, self.Fp), np.float32, -7.5)
        self.norms, self._n = guarded((capacity,), np.float32, -7.5)
        self.cls, self._c = guarded((capacity,), np.int32, -777)
        self.counters, self._k = guarded((3,), np.int64, -7)
        self.bank[:] = 0
        self.norms[:] = 0
        self.cls[:] = 0
        self.counters[:] = 0

    def intact(self):
        assert (self._b[self.cap * self.Fp:] == -7.5).all() and (self._n[self.cap:] == -7.5).all() and (self._c[self.cap:] == -777).all() \
            and (self._k[3:] == -7).all(), 'a write beyond a bank buffer'

    def add(self, levels, classes=None, anchor=None, count=None):
        B = levels[0].shape[0]
        K = anchor.shape[1] if anchor is not None else classes.shape[1]
        nbytes = self.lib.effdet_feature_knn_workspace_bytes(B * K, self.F, 0, 0)
        assert nbytes > 0
        ws = np.full(nbytes + GUARD, 0xA5, np.uint8)
        cdt, cp, cs = 0, 0, 0
        if classes is not None:
            cdt = {np.dtype(np.int32): 0, np.dtype(np.int64): 1, np.dtype(np.float32): 2}[classes.dtype]
            cp, cs = classes.strides[0] // classes.itemsize, classes.strides[1] // classes.itemsize
        rc = self.lib.effdet_feature_knn_append(None, *table(levels), self.F, self.C, self.A, B, K, ptr(anchor), ptr(classes), cdt, cp, cs, 0,
                                                ptr(count), int(count is not None and count.dtype == np.int64), int(self.normalize),
                                                self.every, self.cap, ptr(self.bank), ptr(self.norms), ptr(self.cls), ptr(self.counters),
                                                ptr(ws), nbytes)
        assert rc == 0, rc
        assert (ws[nbytes:] == 0xA5).all(), 'a write beyond the workspace'
        self.intact()

    def score(self, levels, k, splits, anchor=None, count=None, A=None):
        B = levels[0].shape[0]
        A = self.A if A is None else A
        K = anchor.shape[1] if anchor is not None else A * sum(l.shape[1] for l in levels)
        nbytes = self.lib.effdet_feature_knn_workspace_bytes(B * K, self.F, k, splits)
        assert nbytes > 0
        ws = np.full(nbytes + GUARD, 0xA5, np.uint8)
        knn, _a = guarded((B, K), np.float32, -12345.5)
        idx, _i = guarded((B, K), np.int32, -777)
        cls, _c = guarded((B, K), np.int32, -777)
        M = int(self.counters[0])
        rc = self.lib.effdet_feature_knn_score(None, *table(levels), self.F, A, B, K, ptr(anchor), ptr(count),
                                               int(count is not None and count.dtype == np.int64), int(self.normalize), k, splits, M,
                                               ptr(self.bank), ptr(self.norms), ptr(self.cls), ptr(knn), ptr(idx), ptr(cls), ptr(ws), nbytes)
        assert rc == 0, rc
        assert (ws[nbytes:] == 0xA5).all(), 'a write beyond the workspace'
        assert (_a[B * K:] == -12345.5).all() and (_i[B * K:] == -777).all() and (_c[B * K:] == -777).all(), 'a write beyond an output'
        self.intact()
        return knn, idx, cls


def place(rs, x, B, P, A):
    """n rows -> a [B, P, F] pyramid that holds them at shuffled cells, anchors [B, K], count [B] (the last image is short)"""
    n, F = x.shape
    K = -(-n // B)
    pyr = rs.normal(size=(B, P, F)).astype(np.float32)
    cell = np.stack([rs.permutation(P)[:K] for _ in range(B)])
    count = np.clip(n - K * np.arange(B), 0, K).astype(np.int32)
    live = np.arange(K)[None, :] < count[:, None]
    xs = np.zeros((B * K, F), np.float32)
    xs[:n] = x
    pyr[np.arange(B)[:, None].repeat(K, 1)[live], cell[live]] = xs.reshape(B, K, F)[live]
    anchor = (cell * A + rs.randint(0, A, cell.shape)).astype(np.int64)
    return pyr, anchor, count, live


def check_bank(m, ref, name):
    M = int(m.counters[0])
    assert (M, int(m.counters[1]), int(m.counters[2])) == (ref.size, ref.seen, ref.lost), (name, m.counters, ref.size, ref.seen, ref.lost)
    assert np.array_equal(m.cls[:M], ref.classes), name
    if m.normalize:
        ulp = np.spacing(np.abs(ref.rows))
        assert (np.abs(m.bank[:M, :m.F] - ref.rows) <= 2 * ulp).all(), name
        n64 = (m.bank[:M].astype(np.float64) ** 2).sum(1)
        assert (np.abs(m.norms[:M] - n64) <= 1e-6 * n64).all(), name
    else:
        assert np.array_equal(m.bank[:M, :m.F].view(np.uint32), ref.rows.view(np.uint32)), name
        assert np.array_equal(m.norms[:M].view(np.uint32), ref.norms.view(np.uint32)), name
    assert not m.bank[:M, m.F:].any(), name


def run(lib, F, C, normalize):
    A = 3
    rs = np.random.RandomState(F + C)
    d = R.inputs(F, max(C, 1), 200, 70)
    # ---- append: two calls, sampling, overflow; dense against indexed
    for every, cap in ((1, 256), (3, 256), (1, 50)):
        m = Model(lib, F, A, cap, C, normalize, every)
        ref = R.Bank(F, cap, normalize, every)
        for lo, hi in ((0, 77), (77, 200)):
            x, y = d['x_bank'][lo:hi], d['y_bank'][lo:hi].copy()
            if C:
                y[3] = -1
                y[5] = C                                                    # skipped: ignore label, class >= C
            pyr, anchor, count, live = place(rs, x, 2, 150, A)
            K = anchor.shape[1]
            ys = np.full(2 * K, -1, np.int64)
            ys[:len(y)] = y
            ok = live.reshape(-1)[:len(y)] & ((y >= 0) & (y < C) if C else True)
            levels = [pyr[:, :100], pyr[:, 100:]]
            m.add(levels, ys.reshape(2, K) if C else None, anchor, count)
            ref.add(x[ok], y[ok] if C else None)
        check_bank(m, ref, 'F %d C %d every %d capacity %d' % (F, C, every, cap))
    print('F %d C %d normalize %d: append ok (sampling, overflow, two levels)' % (F, C, normalize))
    # ---- score
    for M in (1, 15, 16, 17, 33, 100):
        m = Model(lib, F, A, 128, C, normalize)
        pyr, anchor, count, live = place(rs, d['x_bank'][:M], 1, 120, A)
        yb = d['y_bank'][:M].reshape(1, -1)
        m.add([pyr], yb if C else None, anchor, count)
        assert int(m.counters[0]) == M
        for nq in ((15, 17, 64) if M in (17, 100) else (16, 65) if M == 33 else (17,)):
            xq = d['x_ood'][:nq]
            qp, qa, qc, qlive = place(rs, xq, 2 if nq > 1 else 1, 90, A)
            qc = qc.copy()
            qc[-1] = max(int(qc[-1]) - 2, 0)                                # two rows beyond count
            qlive = np.arange(qa.shape[1])[None, :] < qc[:, None]
            lv = qlive.reshape(-1)[:nq]
            for k in (1, 5):
                ref = R.score(xq, d['x_bank'][:M], k, normalize, d['y_bank'][:M] if C else None)
                f32 = R.score(xq, d['x_bank'][:M], k, normalize, dtype=np.float32)
                e32, bnd = R.bound(ref, f32)
                outs = []
                for splits in (1, 3):
                    knn, idx, cls = m.score([qp], k, splits, qa, qc)
                    outs.append((knn.copy(), idx.copy(), cls.copy()))
                    err = np.abs(knn.reshape(-1)[:nq][lv] - ref['knn'][lv]).max() if lv.any() else 0.0
                    assert err <= bnd, (M, nq, k, splits, err, bnd)
                    ex = R.excluded(ref, bnd)
                    sel = lv & ~ex
                    assert np.array_equal(idx.reshape(-1)[:nq][sel], ref['index'][sel]), (M, nq, k, splits)
                    assert np.array_equal(cls.reshape(-1)[:nq][sel], ref['cls'][sel]), (M, nq, k, splits)
                    assert (knn[~qlive] == 0).all() and (idx[~qlive] == -1).all() and (cls[~qlive] == -1).all()
                    assert (knn[qlive] <= 0).all()
                assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(outs[0], outs[1])), 'splits 1 against 3'
                print('  bank %3d, %2d rows, k %d: error %.2e, E32 %.2e, bound %.2e; splits 1 and 3 bitwise equal' % (M, nq, k, err, e32, bnd))
    # duplicated bank rows: the lower index wins; a query equal to a bank row
    m = Model(lib, F, A, 64, C, normalize)
    x = np.concatenate([d['x_bank'][:20], d['x_bank'][:20]])
    pyr, anchor, count, live = place(rs, x, 1, 60, A)
    m.add([pyr], np.concatenate([d['y_bank'][:20]] * 2).reshape(1, -1) if C else None, anchor, count)
    knn, idx, cls = m.score([pyr], 2, 2, anchor, count)
    assert np.array_equal(idx[0], np.concatenate([np.arange(20)] * 2)), idx
    ref = R.score(x, x, 2, normalize)
    e32, bnd = R.bound(ref, R.score(x, x, 2, normalize, dtype=np.float32))
    assert (np.abs(knn[0]) <= bnd).all() and (knn <= 0).all()
    print('  duplicates: the lower row wins, d2 of a row to itself within %.2e of 0' % bnd)


def main():
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(tmp, 'feature_knn', 'effdet_feature_knn_')
        run(lib, 64, 7, True)
        run(lib, 88, 0, False)
        run(lib, 88, 3, True)
    print('feature_knn on the CPU model: all checks passed')


if __name__ == '__main__':
    main()
