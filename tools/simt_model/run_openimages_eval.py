#!/usr/bin/env python
"""The OpenImages evaluation of csrc/openimages_eval.hip without a GPU: the unit compiled by g++ against the CPU model of common.h
and driven through its C ABI on numpy arrays - the two-stage matching with group-of boxes, the virtual entries, the verified
labels, the append of detection and virtual slots, both sorts, the weighted AP and the pooled AP - against the restatement of
tests/_eval_openimages_ref.py.  Flag words, virtual entries, kept counts, counters, the appended entries and both sorted orders are
compared EXACTLY, AP and pooled AP bitwise.  A guard region follows every buffer.  It checks arithmetic, indexing and bounds, not
timing or the memory model.

    python3 tools/simt_model/run_openimages_eval.py [--quick]    needs g++ with C++20 (std::barrier); minutes, a thread per lane

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

import _eval_openimages_ref as O  # noqa: E402
import run_coco_eval as RC  # noqa: E402
import _model  # noqa: E402
from _model import GUARD  # noqa: E402
from ood_object_detection_amd.effdet.evaluation.openimages_evaluator import parse_openimages_result  # noqa: E402

ptr, guarded, same = RC.ptr, RC.guarded, RC.same


def build(tmp):
    return _model.build(tmp, 'openimages_eval', 'effdet_openimages_', lds=('extern __shared__ int oi_lds[];', 'static int oi_lds[16384];'))   # 64 KiB


def guarded_copy(a, fill):
    """a flat copy of `a` followed by a guard region -> (buffer, check())"""
    if a is None:
        return None, lambda: True
    buf = np.concatenate([a.reshape(-1), np.full(GUARD, fill, a.dtype)])
    ref = buf.copy()
    return buf, lambda: np.array_equal(buf.view(np.uint8), ref.view(np.uint8))


class Model:
    """The calls of OpenImagesDetectionEvaluator on host memory"""

    def __init__(self, lib, C, thresholds, w, pooled, capacity):
        self.lib, self.C, self.cap, self.w, self.pooled = lib, C, capacity, float(w), int(pooled)
        self.T = len(thresholds)
        self.thr = (ctypes.c_float * self.T)(*thresholds)
        self.scores, self.classes = guarded(capacity, np.float32, -7.5), guarded(capacity, np.int32, -77)
        self.words = guarded(capacity, np.uint32, 0xA5A5A5A5)
        self.ws_bytes = lib.effdet_openimages_sorted_workspace_bytes(capacity, C, self.pooled)
        self.res_words = lib.effdet_openimages_sorted_result_bytes(self.T, C) // 8
        assert self.ws_bytes > 0 and self.res_words > 0
        self.ws = np.full(self.ws_bytes // 8 + GUARD, 0x5A5A5A5A5A5A5A5A, np.uint64)
        self.result = guarded(self.res_words, np.int64, -99)
        self.state = np.zeros(4, np.uint32)
        self.counters = guarded(3 * C + self.T * C, np.int32, 0)

    def add_batch(self, det, cnt, gtb, gtc, gtd, gtg, lab):
        B, max_det, _ = det.shape
        M, T, C = gtb.shape[1], self.T, self.C
        assert 0 < self.lib.effdet_openimages_match_lds_bytes(M, C, T) <= 65536
        flags, kept = guarded(B * max_det, np.uint32, 0xA5A5A5A5), guarded(2 * B, np.int32, -5)
        vscore, vflags = guarded(B * M * T, np.float32, -3.5), guarded(B * M * T, np.uint32, 0xA5A5A5A5)
        inputs = [guarded_copy(a, f) for a, f in ((det, 0.5), (cnt, max_det + 100), (gtb, 3.0), (gtc, 1), (gtd, 1), (gtg, 1), (lab, 1))]
        bufs = [b for b, _ in inputs]
        K = 0 if lab is None else lab.shape[1]
        empty = np.zeros(1, np.int64)                                                             # a non-null pointer for a list of length 0
        cn = self.counters
        rc = self.lib.effdet_openimages_match(None, ptr(bufs[0]), ptr(bufs[1]), ptr(bufs[2]), ptr(bufs[3]), ptr(bufs[4]), ptr(bufs[5]),
                                              ptr(empty) if lab is not None and K == 0 else ptr(bufs[6]), K, B, max_det, M, C, self.thr, T,
                                              int(self.w > 0), ptr(flags), ptr(vscore), ptr(vflags), ptr(kept), ptr(cn), ptr(cn[C:]),
                                              ptr(cn[2 * C:]), ptr(cn[3 * C:]))
        assert rc == 0, rc
        assert all(ok() for _, ok in inputs), 'an input changed'
        rc = self.lib.effdet_openimages_append(None, ptr(bufs[0]), ptr(flags), ptr(bufs[3]), ptr(vscore), ptr(vflags), ptr(kept), B,
                                               max_det, M, T, ptr(self.scores), ptr(self.classes), ptr(self.words), self.cap,
                                               ptr(self.state))
        assert rc == 0, rc
        assert (flags[B * max_det:] == 0xA5A5A5A5).all() and (kept[2 * B:] == -5).all(), 'a write beyond a per-batch buffer'
        assert (vscore[B * M * T:] == -3.5).all() and (vflags[B * M * T:] == 0xA5A5A5A5).all(), 'a write beyond the virtual slots'
        assert (cn[3 * C + T * C:] == 0).all(), 'a write beyond the counters'
        assert (self.scores[self.cap:] == -7.5).all() and (self.classes[self.cap:] == -77).all() and (self.words[self.cap:] == 0xA5A5A5A5).all()
        return flags[:B * max_det].reshape(B, max_det), vscore[:B * M * T].reshape(B, M, T), vflags[:B * M * T].reshape(B, M, T), kept[:2 * B].copy()

    def evaluate(self, n=-1):
        C, T, cn = self.C, self.T, self.counters
        rc = self.lib.effdet_openimages_sorted(None, ptr(self.scores), ptr(self.classes), ptr(self.words), self.cap, n, ptr(self.state),
                                               T, C, self.w, self.pooled, ptr(cn), ptr(cn[C:]), ptr(cn[2 * C:]), ptr(cn[3 * C:]),
                                               ptr(self.ws), self.ws_bytes, ptr(self.result))
        assert rc == 0, rc
        assert (self.ws[self.ws_bytes // 8:] == 0x5A5A5A5A5A5A5A5A).all(), 'a write beyond the workspace'
        assert (self.result[self.res_words:] == -99).all(), 'a write beyond the result block'
        return parse_openimages_result(self.result[:self.res_words], T, C)

    def sorted(self, n, pooled=False):
        ws = self.ws.view(np.uint8)
        ko, vo = [self.lib.effdet_openimages_sorted_offset(self.cap, self.C, w + (2 if pooled else 0)) for w in (0, 1)]
        return ws[ko:ko + 8 * n].view(np.uint64), ws[vo:vo + 4 * n].view(np.uint32)


def score_key(scores):
    """the low key word of a float32 score: ascending = score descending"""
    b = (np.asarray(scores, np.float32) + np.float32(0)).view(np.uint32)
    return ~np.where(b & np.uint32(0x80000000), ~b, b ^ np.uint32(0x80000000))


def check_case(lib, name, images, C, M, max_det, thresholds, w, pooled=True, splits=1, capacity=None, need=('absorbed', 'virtual')):
    ref = O.evaluate(images, C, thresholds, w, pooled)
    T = len(thresholds)
    n_virtual = int(sum(((vf & O.INVALID) == 0).sum() for vf in ref['vflags']))
    n_absorbed = int(sum((((f >> 16) & 0x7FFF) != 0).sum() for f in ref['flags']))
    n_dropped = int(sum(((f & O.INVALID) != 0).sum() for f in ref['flags']))
    have = dict(absorbed=n_absorbed, virtual=n_virtual, dropped=n_dropped)
    assert all(have[k] > 0 for k in need), (name, have)
    kept_ref = (ref['words'] & O.INVALID) == 0
    total = int(kept_ref.sum())
    cap = total + 5 if capacity is None else capacity
    m = Model(lib, C, thresholds, w, pooled, cap)
    flags, vs, vf, kept = [], [], [], []
    for idx in np.array_split(np.arange(len(images)), splits):
        f, s, v, k = m.add_batch(*O.pack([images[i] for i in idx], max_det, M))
        flags.append(f), vs.append(s), vf.append(v), kept.append(k[:len(idx)])
    flags, vs, vf, kept = np.concatenate(flags), np.concatenate(vs), np.concatenate(vf), np.concatenate(kept)
    for i, im in enumerate(images):
        n, mm = len(im['det_scores']), len(im['gt_classes'])
        assert np.array_equal(flags[i, :n], ref['flags'][i]), (name, 'flags', i, np.nonzero(flags[i, :n] != ref['flags'][i])[0][:8])
        assert (flags[i, n:] == 0x80000000).all()
        assert np.array_equal(vf[i, :mm], ref['vflags'][i]) and (vf[i, mm:] == 0x80000000).all(), (name, 'vflags', i)
        assert np.array_equal(vs[i, :mm].view(np.uint32), ref['vscore'][i].view(np.uint32)) and (vs[i, mm:] == 0).all(), (name, 'vscore', i)
        assert kept[i] == int(((ref['flags'][i] & O.INVALID) == 0).sum() + ((ref['vflags'][i] & O.INVALID) == 0).sum()), (name, 'kept', i)
    cn = m.counters
    assert np.array_equal(cn[:C], ref['n_plain']) and np.array_equal(cn[C:2 * C], ref['n_group']), (name, 'instance counters')
    assert np.array_equal(cn[2 * C:3 * C], ref['gt_imgs']) and np.array_equal(cn[3 * C:3 * C + T * C].reshape(T, C), ref['correct']), (name, 'corloc')
    live = min(total, cap)
    assert int(m.state[0]) == live and int(m.state[1]) == total - live, (name, m.state, total)
    assert np.array_equal(m.scores[:live], (ref['scores'][kept_ref] + np.float32(0))[:live]), (name, 'appended scores')
    assert np.array_equal(m.classes[:live], ref['classes'][kept_ref][:live]) and np.array_equal(m.words[:live], ref['words'][kept_ref][:live])
    got = m.evaluate()
    assert got['n'] == live and got['lost'] == total - live
    if live == total:
        cls, sc, fl = ref['sorted']
        keys, words = m.sorted(len(cls))
        assert np.array_equal(keys, (cls.astype(np.uint64) << np.uint64(32)) | score_key(sc).astype(np.uint64)), (name, 'sorted keys')
        assert np.array_equal(words, fl), (name, 'sorted words')
        assert same(got['ap'], ref['ap']), (name, 'ap', got['ap'], ref['ap'])
        if pooled:
            pc, ps, pf = ref['pooled']
            pkeys, pwords = m.sorted(len(pc), pooled=True)
            assert np.array_equal(pkeys, score_key(ps).astype(np.uint64)) and np.array_equal(pwords, pf), (name, 'pooled order')
        assert same(got['weighted_ap'], ref['pooled_ap']), (name, 'pooled ap', got['weighted_ap'], ref['pooled_ap'])
    print('%-56s %5d entries; absorbed %4d, virtual %4d, dropped %4d; mAP %.6f pooled %.6f ok'
          % (name, live, n_absorbed, n_virtual, n_dropped, np.nanmean(ref['ap']), np.nanmean(ref['pooled_ap']) if pooled else np.nan))


def main():
    quick = '--quick' in sys.argv[1:]
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(tmp)
        check_case(lib, 'C 3, M 1, T 1, w 1, every box group-of', O.dense_case(1, 2, 3, 1, 12, 1.0, classes_used=1), 3, 1, 14, [0.5], 1.0)
        check_case(lib, 'C 33, M 64, T 3, w 0.5, labels, 2 batches', O.dense_case(2, 3, 33, 64, 60, 0.3, labels=2), 33, 64, 61,
                   [0.5, 0.55, 0.75], 0.5, splits=2, need=('absorbed', 'virtual', 'dropped'))
        check_case(lib, 'C 4, M 40, w 0: absorbed, nothing emitted', O.dense_case(3, 2, 4, 40, 50, 0.5), 4, 40, 50, [0.5, 0.75], 0.0,
                   need=('absorbed',))
        check_case(lib, 'C 4, M 40, w 0.3, virtual entries overflow', O.dense_case(3, 2, 4, 40, 50, 0.5), 4, 40, 50, [0.5, 0.75], 0.3,
                   capacity=int(sum(((f & O.INVALID) == 0).sum() for f in O.evaluate(O.dense_case(3, 2, 4, 40, 50, 0.5), 4, [0.5, 0.75], 0.3)['flags'])) + 3)
        if not quick:
            check_case(lib, 'C 5, M 257, T 15, w 1, no group-of box', O.dense_case(4, 2, 5, 257, 60, 0.0), 5, 257, 60,
                       np.linspace(0.25, 0.95, 15), 1.0, need=())
            check_case(lib, 'C 5, M 300, T 3, w 0.3, every box group-of', O.dense_case(5, 2, 5, 300, 80, 1.0), 5, 300, 100,
                       [0.5, 0.55, 0.75], 0.3)
            check_case(lib, 'C 2, M 257, one class of > 2048 entries', O.dense_case(6, 24, 2, 257, 100, 0.3, classes_used=1), 2, 257, 100,
                       [0.5, 0.75], 0.5, splits=5)


if __name__ == '__main__':
    main()
