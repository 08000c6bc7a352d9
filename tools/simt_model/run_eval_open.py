#!/usr/bin/env python
"""The open-set evaluation of csrc/eval_scale.hip without a GPU: the unit compiled by g++ against the CPU model of common.h and
driven through its C ABI on numpy arrays - matching with C + 1 classes, the open words, the append of both words, the sort with
the second payload, AP and the open-set counts, and the relabelling - against the restatement of tests/_eval_open_ref.py at small
shapes (unknown boxes on both sides of the 256-row LDS chunk, no unknown box, only unknown boxes, images without ground truth or
detections, NaN scores, classes out of range, a class of more than 2048 kept entries (a second chunk in the AP and the counts
kernels, the position in it), entries on both sides of a sort tile).  It checks
arithmetic, indexing and bounds (a guard region follows every buffer), not timing or the memory model.

    python3 tools/simt_model/run_eval_open.py [--quick]    needs g++ with C++20 (std::barrier); minutes, a thread per lane

What the model adds to common.h for this unit: a fixed-size array in place of the matching kernel's dynamic LDS."""
import ctypes
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _eval_open_ref as O  # noqa: E402
import _model  # noqa: E402
from _model import GUARD  # noqa: E402

NAMES = ('effdet_eval_match_multi', 'effdet_eval_open_words', 'effdet_eval_append_open', 'effdet_eval_open_sorted_workspace_bytes',
         'effdet_eval_open_sorted_offset', 'effdet_eval_open_sorted_result_bytes', 'effdet_eval_open_sorted',
         'effdet_eval_ap_sorted_workspace_bytes', 'effdet_eval_ap_sorted_result_bytes', 'effdet_eval_ap_sorted', 'effdet_eval_append',
         'effdet_relabel_unknown', 'effdet_eval_scale_sort_tile')


def build(tmp):
    return _model.build(tmp, 'eval_scale', NAMES, lds=('extern __shared__ int sh[];', 'static int sh[16384];'))


def ptr(a):
    return a.ctypes.data


def guarded(n, dtype, fill):
    return np.full(n + GUARD, fill, dtype)


class Model:
    """The calls of OpenSetDetectionEvaluator on host memory; num_classes counts the unknown class"""

    def __init__(self, lib, num_classes, thresholds, capacity):
        self.lib, self.C1, self.cap = lib, num_classes, capacity
        self.thr = (ctypes.c_float * len(thresholds))(*thresholds)
        self.T = len(thresholds)
        self.scores, self.classes = guarded(capacity, np.float32, -7.5), guarded(capacity, np.int32, -77)
        self.flags, self.open = guarded(capacity, np.uint32, 0xA5A5A5A5), guarded(capacity, np.uint32, 0xA5A5A5A5)
        self.ws_bytes = lib.effdet_eval_open_sorted_workspace_bytes(capacity, num_classes)
        self.res_words = lib.effdet_eval_open_sorted_result_bytes(self.T, num_classes) // 8
        assert self.ws_bytes > 0 and self.res_words > 0
        self.ws = np.full(self.ws_bytes // 8 + GUARD, 0x5A5A5A5A5A5A5A5A, np.uint64)
        self.result = guarded(self.res_words, np.int64, -99)
        self.state = np.zeros(4, np.uint32)
        self.counters = np.zeros(2 * num_classes + self.T * num_classes, np.int32)

    def add_batch(self, det, cnt, gtb, gtc, gtd):
        B, max_det, _ = det.shape
        M, C1 = gtb.shape[1], self.C1
        flags, words = guarded(B * max_det, np.uint32, 0xA5A5A5A5), guarded(B * max_det, np.uint32, 0xA5A5A5A5)
        kept = guarded(2 * B, np.int32, -5)
        g0, g1, g2 = self.counters[:C1], self.counters[C1:2 * C1], self.counters[2 * C1:]
        rc = self.lib.effdet_eval_match_multi(None, ptr(det), ptr(cnt), ptr(gtb), ptr(gtc), ptr(gtd), B, max_det, M, C1, self.thr, self.T,
                                              ptr(flags), ptr(kept), ptr(g0), ptr(g1), ptr(g2))
        assert rc == 0, rc
        rc = self.lib.effdet_eval_open_words(None, ptr(det), ptr(flags), ptr(gtb), ptr(gtc), B, max_det, M, C1, self.thr, self.T, ptr(words))
        assert rc == 0, rc
        rc = self.lib.effdet_eval_append_open(None, ptr(det), ptr(flags), ptr(words), ptr(kept), B, max_det, ptr(self.scores),
                                              ptr(self.classes), ptr(self.flags), ptr(self.open), self.cap, ptr(self.state))
        assert rc == 0, rc
        for a, n in ((flags, B * max_det), (words, B * max_det)):
            assert (a[n:] == 0xA5A5A5A5).all(), 'a write beyond a per-batch buffer'
        assert (kept[2 * B:] == -5).all()
        return flags[:B * max_det].reshape(B, max_det), words[:B * max_det].reshape(B, max_det)

    def evaluate(self, level, n=-1):
        rc = self.lib.effdet_eval_open_sorted(None, ptr(self.scores), ptr(self.classes), ptr(self.flags), ptr(self.open), self.cap, n,
                                              ptr(self.state), self.T, self.C1, ptr(self.counters), ptr(self.counters[self.C1:]),
                                              ptr(self.counters[2 * self.C1:]), level, ptr(self.ws), self.ws_bytes, ptr(self.result))
        assert rc == 0, rc
        assert (self.scores[self.cap:] == -7.5).all() and (self.classes[self.cap:] == -77).all(), 'a write beyond the entries'
        assert (self.flags[self.cap:] == 0xA5A5A5A5).all() and (self.open[self.cap:] == 0xA5A5A5A5).all(), 'a write beyond the entries'
        assert (self.ws[self.ws_bytes // 8:] == 0x5A5A5A5A5A5A5A5A).all(), 'a write beyond the workspace'
        assert (self.result[self.res_words:] == -99).all(), 'a write beyond the result block'
        from ood_object_detection_amd.effdet.evaluation.open_set_evaluator import parse_open_result
        return parse_open_result(self.result[:self.res_words], self.T, self.C1)


def compare(name, got, ref):
    for k in O.MATRICES + ('gt_count', 'gt_imgs', 'correct'):
        assert np.array_equal(got[k], ref[k]), (name, k, got[k], ref[k])
    assert np.array_equal(np.isnan(got['ap']), np.isnan(ref['ap'])), (name, 'AP NaN')
    assert np.allclose(got['ap'], ref['ap'], rtol=0, atol=1e-12, equal_nan=True), (name, 'AP')


def check_case(lib, name, images, C, M, max_det, level, splits=1):
    thresholds = O.CASE_THRESHOLDS
    ref = O.evaluate(images, C, thresholds, level)
    m = Model(lib, C + 1, thresholds, len(images) * max_det + 5)
    flags, words = [], []
    for idx in np.array_split(np.arange(len(images)), splits):
        f, w = m.add_batch(*O.pack([images[i] for i in idx], max_det, M))
        flags.append(f)
        words.append(w)
    flags, words = np.concatenate(flags), np.concatenate(words)
    k = 0
    for i, im in enumerate(images):
        n = len(im['det_scores'])
        assert np.array_equal(flags[i, :n], ref['flags'][k:k + n]), (name, 'flags', i)
        assert np.array_equal(words[i, :n], ref['open'][k:k + n]), (name, 'open words', i)
        assert (flags[i, n:] == 0x80000000).all() and (words[i, n:] == 0).all()
        k += n
    got = m.evaluate(level)
    compare(name, got, ref)
    assert got['n'] == int(((ref['flags'] >> 31) == 0).sum()) and got['lost'] == 0
    print('%-44s %5d entries, A-OSE %s ok' % (name, got['n'], ref['a_ose'].tolist()))


def check_entries(lib, name, n, C1, level, seed, big=0):
    """entries put into the buffers directly: scores with ties, random flag and open words; the first `big` entries are of class 0
    and kept, so that class 0's segment is longer than `big`"""
    rs = np.random.RandomState(seed)
    m = Model(lib, C1, (0.5, 0.75), n + 3)
    scores = (rs.randint(0, 64, n) / np.float32(64)).astype(np.float32)
    classes = rs.randint(-1, C1 + 1, n)
    classes[:big] = 0
    u = rs.uniform(size=n)
    flags = np.where(u < 0.3, 3, np.where(u < 0.4, 1, np.where(u < 0.5, 1 << 17, np.where(u < 0.55, 1 << 31, 0)))).astype(np.uint32)
    flags[:big] &= 0x7FFFFFFF
    words = rs.randint(0, 4, n).astype(np.uint32)
    gt_count = np.array([int(((flags & 1) == 1)[classes == c].sum()) + rs.randint(0, 3) for c in range(C1)])
    gt_count[C1 - 1] = 0
    m.scores[:n], m.classes[:n], m.flags[:n], m.open[:n] = scores, classes, flags, words
    m.state[0] = n
    m.counters[:C1] = gt_count
    got = m.evaluate(level)
    ref = O.counts_from_entries(scores, classes, flags, words, gt_count, C1, 2, level)
    for k in O.MATRICES:
        assert np.array_equal(got[k], ref[k]), (name, k, got[k], ref[k])
    if big:
        import _eval_scale_ref as R
        ap = R.ap_from_entries(scores, classes, flags, gt_count, C1, 2)
        assert np.allclose(got['ap'], ap, rtol=0, atol=1e-12, equal_nan=True), (name, 'AP')
        assert ref['n_det'][0, 0] + 1 > big and ref['pos'][:, 0].min() >= big, (name, 'the position lies in the first chunk')
    print('%-44s %5d entries ok' % (name, n))


def check_relabel(lib):
    rs = np.random.RandomState(3)
    B, max_det, C = 3, 37, 4
    det = rs.uniform(0, 1, (B, max_det, 6)).astype(np.float32)
    det[:, :, 5] = rs.randint(-1, C + 3, (B, max_det))
    det[0, 3, 5], det[0, 7, 5] = 1, 2
    full = rs.normal(0, 1, (B, 2 * max_det)).astype(np.float32)
    score = full[:, ::2]
    score[0, 3], score[1, 4], score[2, 5], tau = np.nan, np.inf, -np.inf, np.float32(score[0, 7])
    count = np.array([max_det, 0, 11], np.int32)
    out = guarded(det.size, np.float32, -3.25)
    tau_dev = np.array([tau], np.float32)
    want = det.copy()
    hit = (np.arange(max_det)[None] < count[:, None]) & (det[:, :, 5] >= 1) & (det[:, :, 5] <= C) & ~(score >= tau)
    want[:, :, 5][hit] = C + 1
    for dev in (None, ptr(tau_dev)):
        rc = lib.effdet_relabel_unknown(None, ptr(det), ptr(count), ptr(score), score.strides[0] // 4, score.strides[1] // 4, B, max_det,
                                        C, float(tau) if dev is None else 123.0, dev, ptr(out))
        assert rc == 0 and np.array_equal(out[:det.size].reshape(det.shape), want) and (out[det.size:] == -3.25).all()
    inplace = det.copy()
    assert lib.effdet_relabel_unknown(None, ptr(inplace), ptr(count), ptr(score), score.strides[0] // 4, score.strides[1] // 4, B,
                                      max_det, C, float(tau), None, ptr(inplace)) == 0
    assert np.array_equal(inplace, want) and hit.any() and not hit[0, 7] and hit[0, 3]
    print('relabel_unknown ok: %d rows became unknown' % int(hit.sum()))


def main():
    quick = '--quick' in sys.argv[1:]
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(tmp)
        tile = lib.effdet_eval_scale_sort_tile()
        check_relabel(lib)
        worked = dict(gt_boxes=np.array([[0, 0, 10, 10], [20, 20, 30, 30]], np.float32), gt_classes=np.array([0, 2]),
                      det_boxes=np.array([[20, 20, 30, 30], [0, 0, 10, 10], [20, 20, 30, 30], [40, 40, 50, 50]], np.float32),
                      det_scores=np.array([0.95, 0.9, 0.7, 0.6], np.float32), det_classes=np.array([0, 0, 2, 1]))
        check_case(lib, 'worked example', [worked], 2, 2, 4, 0.8)
        check_case(lib, 'M 1, no unknown box', O.open_case(1, 4, 12, 5, 1, 0), 5, 1, 12, 0.8)
        check_case(lib, 'M 64, 40 unknown', O.open_case(2, 4, 30, 5, 64, 40), 5, 64, 31, 0.5, splits=2)
        if not quick:
            check_case(lib, 'M 257, 257 unknown', O.open_case(3, 4, 30, 5, 257, 257), 5, 257, 30, 0.625)
            check_case(lib, 'M 300, 257 unknown, 300 detections', O.open_case(4, 4, 300, 5, 300, 257), 5, 300, 300, 0.8, splits=4)
            check_entries(lib, 'tile + 1 entries, 3 classes', tile + 1, 3, 0.625, 11)
        check_entries(lib, '600 entries, 3 classes', 600, 3, 0.8, 12)
        check_entries(lib, '2500 entries, class 0 beyond an AP chunk', 2500, 2, 1.0, 13, big=2049)


if __name__ == '__main__':
    main()
