#!/usr/bin/env python
"""The detection calibration of csrc/calibration_eval.hip without a GPU: the unit compiled by g++ against the CPU model of common.h
and driven through its C ABI on numpy arrays - the matching with the candidate IoU, the append behind the score threshold, both
sorts, the reliability tables, the Newton fit and the apply launch - against the restatement of tests/_calibration_ref.py.  Flag
words, IoU, kept counts, counters, the appended entries, n, tp and the mass-bin boundaries are compared EXACTLY, the float64 sums
within n 2^-52 relative, the fit within 1e-12 with equal iteration and halving counts, apply within one float32 ulp.  A guard
region follows every buffer.  It checks arithmetic, indexing and bounds, not timing or the memory model.

    python3 tools/simt_model/run_calibration_eval.py [--quick]    needs g++ with C++20 (std::barrier); minutes, a thread per lane

What the model adds to common.h for this unit: a fixed-size array in place of the matching kernel's dynamic LDS."""
import ctypes
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _calibration_ref as R  # noqa: E402
import _eval_openimages_ref as O  # noqa: E402
import run_coco_eval as RC  # noqa: E402
import _model  # noqa: E402
from _model import GUARD  # noqa: E402
from ood_object_detection_amd.calibration import _start_state  # noqa: E402
from ood_object_detection_amd.effdet.evaluation.calibration_evaluator import parse_calibration_result  # noqa: E402

ptr, guarded = RC.ptr, RC.guarded


def build(tmp):
    return _model.build(tmp, 'calibration_eval', 'effdet_calibration_', lds=('extern __shared__ int ca_lds[];', 'static int ca_lds[16384];'))   # 64 KiB


class Model:
    """The calls of CalibrationEvaluator and DetectionCalibrator on host memory"""

    def __init__(self, lib, C, thresholds, K, capacity, score_threshold=0.0):
        self.lib, self.C, self.K, self.cap, self.st = lib, C, K, capacity, float(score_threshold)
        self.T = len(thresholds)
        self.thr = (ctypes.c_float * self.T)(*thresholds)
        self.scores, self.classes = guarded(capacity, np.float32, -7.5), guarded(capacity, np.int32, -77)
        self.words, self.iou = guarded(capacity, np.uint32, 0xA5A5A5A5), guarded(capacity, np.float32, -9.5)
        self.ws_bytes = lib.effdet_calibration_workspace_bytes(capacity, C)
        self.res_words = lib.effdet_calibration_result_bytes(self.T, C, K) // 8
        assert self.ws_bytes > 0 and self.res_words > 0
        self.ws = np.full(self.ws_bytes // 8 + GUARD, 0x5A5A5A5A5A5A5A5A, np.uint64)
        self.result = guarded(self.res_words, np.int64, -99)
        self.state = np.zeros(4, np.uint32)
        self.counters = guarded(2 * C + self.T * C, np.int32, 0)

    def add_batch(self, det, cnt, gtb, gtc, gtd):
        B, max_det, _ = det.shape
        M, T, C = gtb.shape[1], self.T, self.C
        flags, iou, kept = guarded(B * max_det, np.uint32, 0xA5A5A5A5), guarded(B * max_det, np.float32, -3.5), guarded(2 * B, np.int32, -5)
        ins = [np.concatenate([a.reshape(-1), np.full(GUARD, f, a.dtype)]) for a, f in ((det, 0.5), (cnt, max_det + 100), (gtb, 3.0), (gtc, 1), (gtd, 1))]
        ref = [a.copy() for a in ins]
        cn = self.counters
        rc = self.lib.effdet_calibration_match(None, ptr(ins[0]), ptr(ins[1]), ptr(ins[2]), ptr(ins[3]), ptr(ins[4]), B, max_det, M, C,
                                               self.thr, T, self.st, ptr(flags), ptr(iou), ptr(kept), ptr(cn), ptr(cn[C:]), ptr(cn[2 * C:]))
        assert rc == 0, rc
        rc = self.lib.effdet_calibration_append(None, ptr(ins[0]), ptr(flags), ptr(iou), ptr(kept), B, max_det, self.st, ptr(self.scores),
                                                ptr(self.classes), ptr(self.words), ptr(self.iou), self.cap, ptr(self.state))
        assert rc == 0, rc
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(ins, ref)), 'an input changed'
        assert (flags[B * max_det:] == 0xA5A5A5A5).all() and (iou[B * max_det:] == -3.5).all() and (kept[2 * B:] == -5).all()
        assert (cn[2 * C + T * C:] == 0).all(), 'a write beyond the counters'
        self.check_entries()
        return flags[:B * max_det].reshape(B, max_det), iou[:B * max_det].reshape(B, max_det), kept[:2 * B].copy()

    def check_entries(self):
        assert (self.scores[self.cap:] == -7.5).all() and (self.classes[self.cap:] == -77).all()
        assert (self.words[self.cap:] == 0xA5A5A5A5).all() and (self.iou[self.cap:] == -9.5).all(), 'a write beyond the entries'

    def table(self, n=-1):
        C, T, cn = self.C, self.T, self.counters
        rc = self.lib.effdet_calibration_table(None, ptr(self.scores), ptr(self.classes), ptr(self.words), ptr(self.iou), self.cap, n,
                                               ptr(self.state), T, C, self.K, ptr(cn), ptr(cn[C:]), ptr(cn[2 * C:]), ptr(self.ws),
                                               self.ws_bytes, ptr(self.result))
        assert rc == 0, rc
        assert (self.ws[self.ws_bytes // 8:] == 0x5A5A5A5A5A5A5A5A).all(), 'a write beyond the workspace'
        assert (self.result[self.res_words:] == -99).all(), 'a write beyond the result block'
        self.check_entries()
        return parse_calibration_result(self.result[:self.res_words], T, C, self.K)

    def fit(self, t, target, method, max_iter=32):
        nb = self.lib.effdet_calibration_fit_workspace_bytes(self.cap)
        part = guarded(nb // 8, np.float64, -1.25)
        st = np.concatenate([np.array(_start_state(), np.float64), np.full(GUARD, -4.5)])
        for _ in range(max_iter):
            rc = self.lib.effdet_calibration_fit_step(None, ptr(self.scores), ptr(self.words), ptr(self.iou), self.cap, ptr(self.state), t,
                                                      int(target == 'iou'), int(method == 'temperature'), ptr(st), ptr(part), nb)
            assert rc == 0, rc
        assert (part[nb // 8:] == -1.25).all() and (st[16:] == -4.5).all(), 'a write beyond the fit blocks'
        return st[:16].copy()


def close(got, ref, n, what):
    """float64 sums of at most n non-negative terms: within n 2^-52 relative"""
    got, ref, n = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(n, np.float64)
    assert (np.abs(got - ref) <= n * 2.0 ** -52 * np.abs(ref)).all(), (what, float(np.abs(got - ref).max()))


def compare_tables(name, got, ref, n_total):
    for k in ('n', 'tp'):
        assert np.array_equal(got['bins'][k], ref['bins'][k]), (name, k)
    assert np.array_equal(got['out_of_range'], ref['out_of_range']) and np.array_equal(got['entries'], ref['entries']), (name, 'counts')
    for k in ('sum_p', 'sum_iou'):
        close(got['bins'][k], ref['bins'][k], np.maximum(got['bins']['n'], 1), (name, k))
    terms = np.maximum(got['bins']['n'][:, :, 0].sum(-1), 1)                  # [T, C + 1]: the scope's entries not ignored at t
    assert int(terms.max()) <= max(n_total, 1)
    for k in ('brier', 'nll'):
        close(got[k], ref[k], terms, (name, k))


def check_images(lib, name, images, C, M, max_det, thresholds, K, score_threshold=0.0, splits=1, capacity=None):
    acc = R.accumulate(images, C, thresholds, score_threshold)
    T, total = len(thresholds), len(acc['scores'])
    cap = total + 5 if capacity is None else capacity
    m = Model(lib, C, thresholds, K, cap, score_threshold)
    flags, ious, kept = [], [], []
    for idx in np.array_split(np.arange(len(images)), splits):
        f, u, k = m.add_batch(*O.pack([images[i] for i in idx], max_det, M)[:5])
        flags.append(f), ious.append(u), kept.append(k[:len(idx)])
    flags, ious, kept = np.concatenate(flags), np.concatenate(ious), np.concatenate(kept)
    for i, im in enumerate(images):
        n = len(im['det_scores'])
        rf, ru = acc['per_image'][i]
        assert np.array_equal(flags[i, :n], rf) and (flags[i, n:] == 0x80000000).all(), (name, 'flags', i)
        assert np.array_equal(ious[i, :n].view(np.uint32), ru.view(np.uint32)) and (ious[i, n:] == 0).all(), (name, 'iou', i)
        with np.errstate(invalid='ignore'):
            want = int((((rf & R.INVALID) == 0) & (np.asarray(im['det_scores'], np.float32) >= np.float32(score_threshold))).sum())
        assert kept[i] == want, (name, 'kept', i)
    cn = m.counters
    assert np.array_equal(cn[:C], acc['gt_count']) and np.array_equal(cn[C:2 * C], acc['gt_imgs']), (name, 'counters')
    assert np.array_equal(cn[2 * C:2 * C + T * C].reshape(T, C), acc['correct']), (name, 'corloc')
    live = min(total, cap)
    assert int(m.state[0]) == live and int(m.state[1]) == total - live and int(m.state[2]) == acc['nan_scores'], (name, m.state, total)
    assert np.array_equal(m.scores[:live], acc['scores'][:live]) and np.array_equal(m.classes[:live], acc['classes'][:live])
    assert np.array_equal(m.words[:live], acc['flags'][:live]) and np.array_equal(m.iou[:live].view(np.uint32), acc['iou'][:live].view(np.uint32))
    got = m.table()
    assert got['n'] == live and got['lost'] == total - live
    assert np.array_equal(got['gt_count'], acc['gt_count']) and np.array_equal(got['correct'], acc['correct'])
    if live == total:
        compare_tables(name, got, R.tables(acc['scores'], acc['classes'], acc['flags'], acc['iou'], C, T, K), total)
    print('%-60s %6d entries, D-ECE %.6f ok' % (name, live, R.metrics(got, 0)['D-ECE']))


def fill(m, scores, classes, flags, iou):
    n = len(scores)
    m.scores[:n], m.classes[:n], m.words[:n], m.iou[:n] = scores, classes, flags, iou
    m.state[:] = (n, 0, 0, 0)


def check_entries(lib, name, counts, T, K, seed, ties=50):
    """entries put into the buffers directly: class c has counts[c] of them, shuffled; scores on a grid of `ties` values"""
    rs = np.random.RandomState(seed)
    C, n = len(counts), int(sum(counts))
    classes = rs.permutation(np.repeat(np.arange(C), counts)).astype(np.int32)
    scores = (rs.randint(0, ties + 1, n) / float(ties)).astype(np.float32)
    tp = rs.randint(0, 1 << T, n).astype(np.uint32)
    ig = rs.randint(0, 1 << T, n).astype(np.uint32) & rs.randint(0, 1 << T, n).astype(np.uint32) & ~tp
    if T == 16:
        ig &= np.uint32(0x7FFF)
    flags = tp | (ig << np.uint32(16))
    iou = rs.uniform(0, 1, n).astype(np.float32)
    m = Model(lib, C, list(np.linspace(0.2, 0.95, T)), K, n + 3)
    fill(m, scores, classes, flags, iou)
    compare_tables(name, m.table(), R.tables(scores, classes.astype(np.int64), flags, iou, C, T, K), n)
    print('%-60s %6d entries ok' % (name, n))


def check_fit(lib, case, target, method):
    n, a0, b0 = R.FIT_CASES[case]
    s, f, u = R.bernoulli_case(100 + case, n, a0, b0)
    f = f | (np.arange(n) % 7 == 0).astype(np.uint32) << np.uint32(17)        # some entries ignored at threshold 1: they take part at 0
    m = Model(lib, 1, [0.5, 0.75], 2, n + 9)
    fill(m, s, np.zeros(n, np.int32), f, u)
    st = m.fit(0, target, method)
    ref = R.newton_fit(*R.fit_data(s, f, u, 0, target), method=method, summation='pairwise')
    assert bool(st[11]) == ref['converged'] and int(st[9]) == ref['iterations'] and int(st[10]) == ref['halvings'], (st, ref)
    assert abs(st[0] - ref['a']) <= 1e-12 and abs(st[1] - ref['b']) <= 1e-12 and int(st[14]) == n, (st, ref)
    print('fit n %6d (%g, %g) %-4s %-12s a %.12f b %.12f in %d evaluations ok' % (n, a0, b0, target, method, st[0], st[1], int(st[9])))
    return st


def check_apply(lib, a, b):
    rs = np.random.RandomState(4)
    B, max_det = 3, 300
    det = rs.uniform(0, 1, (B, max_det, 6)).astype(np.float32)
    det[:, :, 4] = -np.sort(-det[:, :, 4], axis=1)
    det[0, 0, 4], det[0, 1, 4], det[1, 5, 4] = 1.0, 0.0, np.nan
    cnt = np.array([300, 17, 0], np.int32)
    din, out = np.concatenate([det.reshape(-1), np.full(GUARD, 0.5, np.float32)]), guarded(det.size, np.float32, -2.5)
    st = np.array(_start_state(a, b), np.float64)
    assert lib.effdet_calibration_apply(None, ptr(din), ptr(cnt), ptr(st), B, max_det, ptr(out)) == 0
    assert (out[det.size:] == -2.5).all(), 'a write beyond det_out'
    got, ref = out[:det.size].reshape(det.shape), R.apply_det(det, cnt, a, b)
    mask = np.ones(det.shape, bool)
    for i in range(B):
        mask[i, :cnt[i], 4] = False
    assert np.array_equal(got[mask].view(np.uint32), det[mask].view(np.uint32)), 'apply changed what it should copy'
    g, r = got[~mask], ref[~mask]
    ok = np.isnan(r) & np.isnan(g) | (np.abs(g.view(np.int32).astype(np.int64) - r.view(np.int32).astype(np.int64)) <= 1)
    assert ok.all(), 'apply differs by more than one float32 ulp'
    print('apply (%g, %g) ok' % (a, b))


def main():
    quick = '--quick' in sys.argv[1:]
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(tmp)
        check_images(lib, 'C 3, M 1, T 1, K 1', O.dense_case(1, 2, 3, 1, 12, 0.0, classes_used=1), 3, 1, 14, [0.5], 1)
        check_images(lib, 'C 4, M 40, T 2, K 15, difficult, score threshold 0.3, 2 batches', O.dense_case(3, 3, 4, 40, 50, 0.0, difficult_frac=0.3),
                     4, 40, 50, [0.5, 0.75], 15, score_threshold=0.3, splits=2)
        check_images(lib, 'C 4, M 40, T 2, K 5, overflow', O.dense_case(3, 2, 4, 40, 50, 0.0), 4, 40, 50, [0.5, 0.75], 5, capacity=20)
        check_entries(lib, 'C 3, K 4, counts 1 / 2047 / 2049', [1, 2047, 2049], 2, 4, 11)
        check_fit(lib, 0, 'tp', 'platt')
        check_fit(lib, 0, 'iou', 'temperature')
        check_apply(lib, 1.5, -0.5)
        if not quick:
            check_images(lib, 'C 5, M 300, T 16, K 64', O.dense_case(5, 2, 5, 300, 80, 0.0), 5, 300, 100, np.linspace(0.2, 0.95, 16), 64)
            check_entries(lib, 'C 7, K 15, counts around 2048 and 4096', [1, 2047, 2048, 2049, 4095, 4096, 4097], 1, 15, 12)
            check_entries(lib, 'C 2, K 64, T 16, one class of 9000', [9000, 0], 16, 64, 13, ties=9)
            check_fit(lib, 1, 'tp', 'platt')
            check_fit(lib, 1, 'iou', 'platt')
            check_fit(lib, 3, 'tp', 'temperature')
            check_apply(lib, 0.05, 2.0)


if __name__ == '__main__':
    main()
