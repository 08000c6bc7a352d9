#!/usr/bin/env python
"""csrc/ood_eval.hip without a GPU: the unit compiled by g++ against the CPU model of common.h and driven through its C ABI on
numpy arrays - append (counts, score filter, negation, strided views, overflow), the radix sort and the metrics - against the
float64 restatement of tests/_ood_eval_ref.py, at the small shapes of tests/test_ood_eval_gpu.py (tile boundaries, ties, one
value everywhere, digit isolation, special values).  It checks arithmetic, indexing and bounds (a guard region follows every
buffer), not timing or the memory model.

    python3 tools/simt_model/run_ood_eval.py [--quick]    needs g++ with C++20 (std::barrier); ten minutes or so, a thread per lane
                                                          (--quick: without the tile-boundary, tie and digit shapes)"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _ood_eval_ref as R  # noqa: E402
from _model import GUARD, build  # noqa: E402

SENTINEL = np.float32(-12345.5)


def ptr(a, offset=0):
    return a.ctypes.data + offset


class Model:
    """The calls of ood.OODEvaluator on host memory"""

    def __init__(self, lib, cap_in, cap_ood):
        self.lib, self.cap = lib, (cap_in, cap_ood)
        self.bufs = [np.full(c + GUARD, SENTINEL, np.float32) for c in self.cap]
        self.ws_bytes = lib.effdet_ood_eval_workspace_bytes(cap_in, cap_ood)
        assert self.ws_bytes > 0
        self.ws = np.full(self.ws_bytes + 4 * GUARD, 0xA5, np.uint8)
        self.state = np.zeros(4, np.uint32)
        self.result = np.zeros(12, np.uint64)

    def add(self, scores, ood, count=None, det=None, min_score=0.0, negate=False):
        s = scores.reshape(1, -1) if scores.ndim == 1 else scores
        B, K = s.shape
        side = 1 if ood else 0
        rc = self.lib.effdet_ood_eval_append(
            None, ptr(s), s.strides[0] // 4, s.strides[1] // 4, B, K, None if count is None else ptr(count),
            int(count is not None and count.dtype == np.int64), None if det is None else ptr(det),
            0 if det is None else det.strides[0] // 4, 0 if det is None else det.strides[1] // 4, min_score, int(negate),
            ptr(self.bufs[side]), self.cap[side], ptr(self.state, 8 * side), ptr(self.ws), self.ws_bytes)
        assert rc == 0, rc

    def evaluate(self, level=0.95):
        rc = self.lib.effdet_ood_eval_sort(None, ptr(self.bufs[0]), self.cap[0], ptr(self.bufs[1]), self.cap[1], ptr(self.state),
                                           ptr(self.ws), self.ws_bytes)
        assert rc == 0, rc
        rc = self.lib.effdet_ood_eval_metrics(None, self.cap[0], self.cap[1], ptr(self.state), ptr(self.ws), self.ws_bytes, level,
                                              ptr(self.result))
        assert rc == 0, rc
        for b, c in zip(self.bufs, self.cap):
            assert (b[c:] == SENTINEL).all(), 'a write beyond a score buffer'
        assert (self.ws[self.ws_bytes:] == 0xA5).all(), 'a write beyond the workspace'
        r = self.result
        P, N, gt, eq, tp, fp, flags = (int(v) for v in r[:7])
        out = {'n_in': P, 'n_ood': N, 'pairs_gt': gt, 'pairs_eq': eq, 'tp': tp, 'fp': fp, 'flags': flags,
               'aupr_in': float(r[8:9].view(np.float64)[0]), 'aupr_out': float(r[9:10].view(np.float64)[0]),
               'threshold': float(r[10:11].view(np.float32)[0])}
        if P and N:
            out['auroc'] = (gt + 0.5 * eq) / (P * N)
        off = [self.lib.effdet_ood_eval_sorted_offset(*self.cap, s) for s in (0, 1)]
        out['sorted'] = [self.ws[o:o + 4 * n].view(np.float32).copy() for o, n in zip(off, (P, N))]
        return out


def check(lib, name, pos, neg, level=0.95, slack=0):
    pos, neg = np.ascontiguousarray(pos, np.float32), np.ascontiguousarray(neg, np.float32)
    m = Model(lib, pos.size + slack, neg.size + slack)
    m.add(pos, False)
    m.add(neg, True)
    got, ref = m.evaluate(level), R.metrics(pos, neg, level)
    assert got['flags'] == 0, (name, got['flags'])
    for k in R.INT_KEYS + ('threshold',):
        assert got[k] == ref[k], (name, k, got[k], ref[k])
    for side, x in enumerate((pos, neg)):
        assert np.array_equal(got['sorted'][side].view(np.uint32), np.sort(R.canonical(x)).view(np.uint32)), (name, 'sorted', side)
    assert abs(got['auroc'] - ref['auroc']) <= 1e-12
    e_in, e_out = abs(got['aupr_in'] - ref['aupr_in']), abs(got['aupr_out'] - ref['aupr_out'])
    assert e_in <= R.aupr_bound(ref['groups_in']) and e_out <= R.aupr_bound(ref['groups_out']), (name, e_in, e_out)
    print('%-34s P %6d N %6d ok (aupr deviation %.1e / %.1e)' % (name, pos.size, neg.size, e_in, e_out))


def bits(b, sign, rs, n):
    """float32 patterns in which only byte b varies (exponent kept finite), with the given sign bit"""
    base = np.uint32(0x3F000000 if b != 3 else 0x00400000)
    v = (rs.randint(0, 256 if b != 3 else 127, n).astype(np.uint32) << np.uint32(8 * b))
    x = (base & ~np.uint32(0xFF << (8 * b)) | v) & np.uint32(0x7FFFFFFF)
    return (x | np.uint32(sign << 31)).view(np.float32)


def main():
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(tmp, 'ood_eval', 'effdet_ood_eval_')
        T = lib.effdet_ood_eval_sort_tile()
        rs = np.random.RandomState(0)
        check(lib, 'one each, >', [1.0], [0.5])
        check(lib, 'one each, ==', [0.5], [0.5])
        check(lib, '-0.0 against +0.0', [-0.0], [0.0])
        check(lib, '1 x 5', [0.3], rs.normal(0, 1, 5))
        if '--quick' not in sys.argv[1:]:
            check(lib, 'tile - 1 / tile + 1, shifted', rs.normal(0.4, 1, T - 1), rs.normal(0, 1, T + 1), slack=3)
            check(lib, 'tile / 3 tiles + 17', rs.normal(0, 1, T), rs.normal(0, 1, 3 * T + 17))
            check(lib, 'halves', np.round(rs.normal(0.4, 1, 2 * T + 5) * 2) / 2, np.round(rs.normal(0, 1, T + 9) * 2) / 2, level=0.5)
            check(lib, 'all equal', np.full(3 * T + 17, 0.25), np.full(2 * T + 5, 0.25))
            for b in range(4):
                x = np.concatenate([bits(b, 0, rs, 700), bits(b, 1, rs, 700)])
                y = np.concatenate([bits(b, 0, rs, 300), bits(b, 1, rs, 300)])
                check(lib, 'only byte %d varies' % b, x, y)
        sp = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 3.4028235e38, -3.4028235e38, 1.0, -1.0], np.float32)
        check(lib, 'special values', sp, sp[::-1][:7], level=1.0)
        check(lib, 'smallest level', rs.normal(0, 1, 300), rs.normal(0, 1, 200), level=1e-9)

        # accumulation: counts of 0 and K, a score filter, negation, strided views, int64 counts
        B, K = 6, 37
        full = rs.normal(0, 1, (B, 2 * K)).astype(np.float32)
        view = full[:, ::2]                                            # a strided view
        det = rs.uniform(0, 1, (B, K, 6)).astype(np.float32)
        count = np.array([0, K, 5, 36, 1, K], np.int32)
        keep = (np.arange(K)[None, :] < count[:, None]) & (det[:, :, 4] >= 0.3)
        m = Model(lib, 4 * B * K, 4 * B * K)
        m.add(view, False, count=count, det=det[:, :, 4], min_score=0.3, negate=True)
        m.add(view, True, count=count.astype(np.int64))
        m.add(full[0], False)
        m.add(full[1:3], True)
        pos = np.concatenate([-view[keep], full[0]])
        neg = np.concatenate([view[np.arange(K)[None, :] < count[:, None]], full[1:3].reshape(-1)])
        n_pos = int(m.state[0])
        assert np.array_equal(m.bufs[0][:n_pos], pos) and np.array_equal(m.bufs[1][:int(m.state[2])], neg), 'append order'
        got, ref = m.evaluate(), R.metrics(pos, neg)
        assert all(got[k] == ref[k] for k in R.INT_KEYS + ('threshold',)) and got['flags'] == 0
        print('accumulation in (b, j) order ok: %d and %d scores' % (pos.size, neg.size))

        # overflow, NaN and an empty side are flagged, and nothing is written beyond a buffer
        m = Model(lib, 99, 50)
        m.add(rs.normal(0, 1, 60).astype(np.float32), False)
        m.add(rs.normal(0, 1, 40).astype(np.float32), False)
        x = rs.normal(0, 1, 50).astype(np.float32)
        x[17] = np.nan
        m.add(x, True)
        got = m.evaluate()
        assert got['flags'] == 2 | 4 and got['n_in'] == 99, got['flags']
        m = Model(lib, 10, 10)
        m.add(rs.normal(0, 1, 4).astype(np.float32), False)
        assert m.evaluate()['flags'] == 32
        print('overflow, NaN and empty-side flags ok')


if __name__ == '__main__':
    main()
