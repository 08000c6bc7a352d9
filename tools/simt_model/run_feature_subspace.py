#!/usr/bin/env python
"""csrc/feature_subspace.hip without a GPU: the unit compiled by g++ against the CPU model of common.h (which models the
float32-input MFMA as the fmaf chain it is) and driven through its C ABI on numpy arrays - score and calibrate at F = 64 and 88,
F - D in {1, 44, F}, 1 .. 65 rows - against the restatement of tests/_feature_subspace_ref.py.  It checks arithmetic, indexing and
bounds (a guard region follows every buffer), not timing or the memory model.

    python3 tools/simt_model/run_feature_subspace.py     needs g++ with C++20 (std::barrier); a thread per lane: about half a minute"""
import ctypes
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _feature_subspace_ref as R  # noqa: E402
from _model import GUARD, build, guarded, ptr  # noqa: E402
from ood_object_detection_amd.ood_features import finalize_subspace  # noqa: E402

A = 3


def lls(v):
    return (ctypes.c_longlong * len(v))(*[int(x) for x in v])


def table(levels):
    es = levels[0].itemsize
    return (0 if es == 4 else 1, len(levels), (ctypes.c_void_p * len(levels))(*[l.ctypes.data for l in levels]),
            lls([l.shape[1] for l in levels]), lls([l.strides[0] // es for l in levels]), lls([l.strides[1] // es for l in levels]),
            lls([l.strides[2] // es for l in levels]))


class Model:
    """The device calls of ood_features.SubspaceFeatureOOD on host memory; q: the float32 parameters of `_feature_subspace_ref.params`"""

    def __init__(self, lib, F, q):
        self.lib, self.F = lib, F
        Rn = q['Rt'].shape[0]
        Fp, Rp = (F + 15) // 16 * 16, (Rn + 15) // 16 * 16
        self.Rt, self._Rt = guarded((Rp, Fp), np.float32, 0)
        self.il, self._il = guarded((Rp,), np.float32, 0)
        self.mu0, self._mu0 = guarded((Fp,), np.float32, 0)
        self._Rt[Rp * Fp:] = self._il[Rp:] = self._mu0[Fp:] = np.nan            # a read beyond a parameter poisons the row
        self.Rt[:Rn, :F], self.il[:Rn], self.mu0[:F] = q['Rt'], q['inv_lambda'], q['mu0']
        self.Rp = Rp
        self.n, self._n = guarded((1,), np.int64, -7)
        self.sums, self._s = guarded((2,), np.float64, -7.5)
        self.n[:] = 0
        self.sums[:] = 0

    def score(self, levels, anchor=None, count=None, A_=A, logit=None, negate=1, alpha=0.0):
        B = levels[0].shape[0]
        K = anchor.shape[1] if anchor is not None else A_ * sum(l.shape[1] for l in levels)
        outs = [guarded((B, K), np.float32, -12345.5) for _ in range(3)]
        (res, _r), (pm, _p), (vim, _v) = outs
        es = 4
        rc = self.lib.effdet_feature_subspace_score(None, *table(levels), self.F, A_, B, K, ptr(anchor), ptr(count),
                                                    int(count is not None and count.dtype == np.int64), ptr(self.Rt), ptr(self.il),
                                                    ptr(self.mu0), self.Rp, ptr(logit), 0 if logit is None else logit.strides[0] // es,
                                                    0 if logit is None else logit.strides[1] // es, negate, alpha, ptr(res), ptr(pm),
                                                    None if logit is None else ptr(vim))
        assert rc == 0, rc
        assert all((w[B * K:] == -12345.5).all() for _, w in outs), 'a write beyond an output'
        if logit is None:
            assert (vim == -12345.5).all(), 'vim written without a logit score'
        return res, pm, vim

    def calibrate(self, levels, anchor, count, logit, negate=1):
        B, K = anchor.shape
        nbytes = self.lib.effdet_feature_subspace_workspace_bytes(B * K)
        assert nbytes > 0
        ws = np.full(nbytes + GUARD, 0xA5, np.uint8)
        rc = self.lib.effdet_feature_subspace_calibrate(None, *table(levels), self.F, A, B, K, ptr(anchor), ptr(count),
                                                        int(count.dtype == np.int64), ptr(self.Rt), ptr(self.mu0), self.Rp, ptr(logit),
                                                        logit.strides[0] // 4, logit.strides[1] // 4, negate, ptr(self.n), ptr(self.sums),
                                                        ptr(ws), nbytes)
        assert rc == 0, rc
        assert (ws[nbytes:] == 0xA5).all(), 'a write beyond the workspace'
        assert (self._n[1:] == -7).all() and (self._s[2:] == -7.5).all(), 'a write beyond a counter'
        assert self.lib.effdet_feature_subspace_calibrate(None, *table(levels), self.F, A, B, K, ptr(anchor), ptr(count), 0, ptr(self.Rt),
                                                          ptr(self.mu0), self.Rp, ptr(logit), K, 1, negate, ptr(self.n), ptr(self.sums),
                                                          ptr(ws), nbytes - 256) == -22


def place(x, B, rs):
    """n rows -> a [B, P, F] pyramid with them at shuffled cells, anchors [B, K], count [B] (the last image holds the remainder)"""
    n, F = x.shape
    K = -(-n // B)
    P = K + 5
    pyr = rs.normal(size=(B, P, F)).astype(np.float32)
    cell = np.stack([rs.permutation(P)[:K] for _ in range(B)])
    count = np.clip(n - K * np.arange(B), 0, K).astype(np.int32)
    xs = np.zeros((B * K, F), np.float32)
    xs[:n] = x
    live = np.arange(K)[None, :] < count[:, None]
    pyr[np.arange(B)[:, None].repeat(K, 1)[live], cell[live]] = xs.reshape(B, K, F)[live]
    anchor = (cell * A + rs.randint(0, A, cell.shape)).astype(np.int64)
    return pyr, anchor, count, live


def run(lib, F, Rn):
    d = R.inputs(F, 400, 65)
    q = R.params(finalize_subspace(*R.stats(d['x_fit']), dim=F - Rn))
    m = Model(lib, F, q)
    rs = np.random.RandomState(F + Rn)
    alpha = 0.75
    worst = {k: 0.0 for k in R.KEYS}
    # the bound comes from the whole case of 65 rows: the E32 of a handful of rows is a noisy sample of the same quantity
    full = R.score(d['x_ood'], q, logit=d['logit'][:65], alpha=alpha)
    bnd = R.bounds(full, R.score(d['x_ood'], q, np.float32, logit=d['logit'][:65], alpha=alpha))
    for n, B in ((1, 1), (15, 1), (16, 1), (17, 2), (63, 1), (64, 2), (65, 3)):
        x = d['x_ood'][:n]
        pyr, anchor, count, live = place(x, B, rs)
        K = anchor.shape[1]
        wide = np.full((B, 2 * K + 1), 777.0, np.float32)
        logit = wide[:, 1::2]                                             # a strided view
        logit[live] = d['logit'][:n]
        levels = [pyr[:, :3], pyr[:, 3:]]                                 # two views of one buffer
        res, pm, vim = m.score(levels, anchor, count, logit=logit, alpha=alpha)
        ref = {k: full[k][:n] for k in R.KEYS}
        for k, got in zip(R.KEYS, (res, pm, vim)):
            err = np.abs(got[live] - ref[k]).max()
            assert err <= bnd[k][1], (F, Rn, n, k, err, bnd[k])
            assert (got[~live] == 0).all(), (F, Rn, n, k)
            worst[k] = max(worst[k], err / bnd[k][1])
        # vim is the two roundings of its formula on the device's own r, bit for bit; max_logit keeps the sign
        r32 = -res[live]
        assert np.array_equal(vim[live].view(np.uint32), (-d['logit'][:n] - np.float32(alpha) * r32).view(np.uint32))
        _, _, vim_m = m.score(levels, anchor, count, logit=logit, negate=0, alpha=alpha)
        assert np.array_equal(vim_m[live].view(np.uint32), (d['logit'][:n] - np.float32(alpha) * r32).view(np.uint32))
        # no logit score: the same residual and partial, vim untouched
        res2, pm2, _ = m.score(levels, anchor, count)
        assert np.array_equal(res2.view(np.uint32), res.view(np.uint32)) and np.array_equal(pm2.view(np.uint32), pm.view(np.uint32))
        # one packed level, int64 counts -> bitwise
        res3, pm3, _ = m.score([pyr], anchor, count.astype(np.int64))
        assert np.array_equal(res3.view(np.uint32), res.view(np.uint32)) and np.array_equal(pm3.view(np.uint32), pm.view(np.uint32))
        # every cell against the identity index with A = 1 -> bitwise; and against the indexed rows
        P = pyr.shape[1]
        c_r, c_p, _ = m.score(levels, A_=1)
        i_r, i_p, _ = m.score([pyr], np.tile(np.arange(P, dtype=np.int64), (B, 1)), A_=1)
        assert np.array_equal(c_r.view(np.uint32), i_r.view(np.uint32)) and np.array_equal(c_p.view(np.uint32), i_p.view(np.uint32))
        cell = anchor // A
        assert np.array_equal(c_r[np.arange(B)[:, None], cell][live].view(np.uint32), res[live].view(np.uint32))
        # bfloat16 features against their float32 widening -> bitwise
        bits = (pyr.view(np.uint32) >> 16).astype(np.uint16)
        b_r, b_p, _ = m.score([bits], anchor, count)
        w_r, w_p, _ = m.score([R.widen_bf16(bits)], anchor, count)
        assert np.array_equal(b_r.view(np.uint32), w_r.view(np.uint32)) and np.array_equal(b_p.view(np.uint32), w_p.view(np.uint32))
        # calibrate: n exact, the sums of the device's own r and t in float64
        before = (int(m.n[0]), m.sums.copy())
        m.calibrate(levels, anchor, count, logit)
        assert int(m.n[0]) - before[0] == n
        st, sr = (-d['logit'][:n].astype(np.float64)).sum(), r32.astype(np.float64).sum()
        tol = n * 2.0 ** -50
        assert abs((m.sums[0] - before[1][0]) - st) <= tol * max(np.abs(d['logit'][:n]).sum(), 1.0) + 1e-12 * abs(before[1][0])
        assert abs((m.sums[1] - before[1][1]) - sr) <= tol * max(sr, 1.0) + 1e-12 * abs(before[1][1])
    print('F %3d, F - D %3d: score and calibrate ok; worst error / bound: %s' % (F, Rn, ', '.join('%s %.2f' % kv for kv in worst.items())))


def refusals(lib):
    d = R.inputs(64, 100, 4)
    q = R.params(finalize_subspace(*R.stats(d['x_fit']), dim=32))
    m = Model(lib, 64, q)
    pyr = np.zeros((1, 4, 64), np.float32)
    out = np.zeros((1, 4), np.float32)
    t = table([pyr])

    def call(F=64, A_=1, B=1, K=4, Rp=32, vim=None, logit=None):
        return lib.effdet_feature_subspace_score(None, *t, F, A_, B, K, None, None, 0, ptr(m.Rt), ptr(m.il), ptr(m.mu0), Rp, logit, 4, 1, 1, 0.5,
                                                 ptr(out), ptr(out), vim)
    assert call() == 0
    for kw in (dict(F=65), dict(A_=0), dict(K=0), dict(Rp=0), dict(Rp=24), dict(Rp=80), dict(vim=ptr(out)), dict(B=1 << 14, K=1 << 14)):
        assert call(**kw) == -22, kw
    assert lib.effdet_feature_subspace_workspace_bytes(0) == -22 and lib.effdet_feature_subspace_workspace_bytes((1 << 27) + 1) == -22
    print('refusals ok')


def main():
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(tmp, 'feature_subspace', 'effdet_feature_subspace_')
        refusals(lib)
        for F in (64, 88):
            for Rn in (1, 44, F):
                run(lib, F, Rn)
    print('feature_subspace on the CPU model: all checks passed')


if __name__ == '__main__':
    main()
