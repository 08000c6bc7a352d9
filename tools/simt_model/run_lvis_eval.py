#!/usr/bin/env python
"""The LVIS federated matching of csrc/lvis_eval.hip without a GPU: the unit compiled by g++ against the CPU model of common.h and
driven through its C ABI on numpy arrays - validity, the image rank with ties, the cap, the federated filter, the bitsets at the
word edges of C, matching in rank order, the not-exhaustive rule - against the restatement of tests/_lvis_eval_ref.py.  Flag words,
ranks, kept counts and npig are compared EXACTLY; the append, the sort and AP / AR then run on the model of csrc/coco_eval.hip
(tools/simt_model/run_coco_eval.py) and precision, AP and AR are compared bitwise.  A guard region follows every buffer, the lists
included.  It checks arithmetic, indexing and bounds, not timing or the memory model.

    python3 tools/simt_model/run_lvis_eval.py [--quick]    needs g++ with C++20 (std::barrier); minutes, a thread per lane

What the model adds to common.h for this unit: a fixed-size array in place of the kernel's dynamic LDS."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _lvis_eval_ref as L  # noqa: E402
import run_coco_eval as RC  # noqa: E402
import _model  # noqa: E402
from _model import GUARD  # noqa: E402


def build(tmp):
    return _model.build(tmp, 'lvis_eval', 'effdet_lvis_match', lds=('extern __shared__ double lv_lds[];', 'static double lv_lds[8192];'))   # 64 KiB


def guarded_copy(a, fill):
    """a flat copy of `a` followed by a guard region -> (buffer, check())"""
    if a is None:
        return None, lambda: True
    buf = np.concatenate([a.reshape(-1), np.full(GUARD, fill, a.dtype)])
    ref = buf.copy()
    return buf, lambda: np.array_equal(buf.view(np.uint8), ref.view(np.uint8))


class Model(RC.Model):
    """The calls of LvisDetectionEvaluator on host memory: the match of the LVIS unit, everything else of the COCO unit"""

    def __init__(self, lvis_lib, coco_lib, *args, **kw):
        super().__init__(coco_lib, *args, **kw)
        self.lvis = lvis_lib

    def add_batch(self, det, cnt, gtb, gtc, area, neg, nel):
        B, max_det, _ = det.shape
        M, A = gtb.shape[1], self.A
        assert self.lvis.effdet_lvis_match_lds_bytes(max_det, M, self.C) <= 8192 * 8
        flags, rank = RC.guarded(B * max_det * A, np.uint32, 0xA5A5A5A5), RC.guarded(B * max_det, np.int32, -5)
        kept = RC.guarded(2 * B, np.int32, -5)
        inputs = [guarded_copy(a, f) for a, f in ((det, 0.5), (cnt, max_det + 100), (gtb, 3.0), (gtc, 1), (area, 5.0), (neg, 1), (nel, 1))]
        bufs = [b for b, _ in inputs]
        empty = np.zeros(1, np.int64)                                                             # a non-null pointer for a list of length 0
        Kn, Ke = (0 if neg is None else neg.shape[1]), (0 if nel is None else nel.shape[1])
        rc = self.lvis.effdet_lvis_match(None, RC.ptr(bufs[0]), RC.ptr(bufs[1]), RC.ptr(bufs[2]), RC.ptr(bufs[3]), RC.ptr(bufs[4]), B,
                                         max_det, M, self.C, self.thr, self.T, self.areas, A, self.max_dets[self.Mx - 1], self.min_score,
                                         RC.ptr(empty) if neg is not None and Kn == 0 else RC.ptr(bufs[5]), Kn,
                                         RC.ptr(empty) if nel is not None and Ke == 0 else RC.ptr(bufs[6]), Ke,
                                         RC.ptr(flags), RC.ptr(rank), RC.ptr(kept), RC.ptr(self.npig))
        assert rc == 0, rc
        assert all(ok() for _, ok in inputs), 'an input changed'
        rc = self.lib.effdet_coco_append(None, RC.ptr(det), RC.ptr(flags), RC.ptr(rank), RC.ptr(kept), B, max_det, A, RC.ptr(self.scores),
                                         RC.ptr(self.classes), RC.ptr(self.words), RC.ptr(self.ranks), self.cap, RC.ptr(self.state))
        assert rc == 0, rc
        assert (flags[B * max_det * A:] == 0xA5A5A5A5).all() and (rank[B * max_det:] == -5).all(), 'a write beyond a per-batch buffer'
        assert (kept[2 * B:] == -5).all() and (self.npig[self.C * A:] == 0).all(), 'a write beyond kept or npig'
        return flags[:B * max_det * A].reshape(B, max_det, A), rank[:B * max_det].reshape(B, max_det), kept[:2 * B].copy()


def check_case(libs, name, images, C, M, max_det, thresholds=L.LVIS_THRESHOLDS, areas=L.LVIS_AREAS, max_dets=L.LVIS_MAX_DETS,
               rec_thr=L.LVIS_REC_THRS, splits=1, min_score=0.0, Kn=None, need=('cut', 'filtered', 'nel')):
    ref = L.evaluate(images, C, thresholds, areas, max_dets, rec_thr, min_score)
    assert all(ref['stats'][k] > 0 for k in need), (name, ref['stats'])
    m = Model(libs[0], libs[1], C, thresholds, areas, max_dets, rec_thr, len(images) * max_det + 5, min_score)
    flags, ranks, kept = [], [], []
    for idx in np.array_split(np.arange(len(images)), splits):
        f, r, k = m.add_batch(*L.pack([images[i] for i in idx], max_det, M, Kn=Kn))
        flags.append(f)
        ranks.append(r)
        kept.append(k[:len(idx)])
    flags, ranks, kept = np.concatenate(flags), np.concatenate(ranks), np.concatenate(kept)
    for i, im in enumerate(images):
        n = len(im['det_scores'])
        assert np.array_equal(flags[i, :n], ref['flags'][i]), (name, 'flags', i, flags[i, :n], ref['flags'][i])
        assert np.array_equal(ranks[i, :n], ref['ranks'][i]), (name, 'ranks', i)
        assert (flags[i, n:] == 0x80000000).all() and (ranks[i, n:] == -1).all()
        assert kept[i] == int((ref['ranks'][i] >= 0).sum()), (name, 'kept', i)
    n = len(ref['scores'])
    assert np.array_equal(m.scores[:n], ref['scores'] + np.float32(0)) and np.array_equal(m.classes[:n], ref['classes'])
    got = m.evaluate()
    RC.compare(name, got, ref, m, n)
    print('%-50s %5d entries; cut %4d, filtered %4d, nel-ignored %4d; AP %.6f ok'
          % (name, n, ref['stats']['cut'], ref['stats']['filtered'], ref['stats']['nel'], np.nanmean(ref['ap'][:, :, 0, -1])))


def main():
    quick = '--quick' in sys.argv[1:]
    with tempfile.TemporaryDirectory() as tmp:
        libs = (build(tmp), RC.build(tmp))
        check_case(libs, 'C 3, M 1, T 1, A 1, cap 6', L.random_images(1, 3, 3, 1, 12, n_neg=1), 3, 1, 12, thresholds=[0.5], areas=[L.LVIS_AREAS[0]],
                   max_dets=(6,))
        check_case(libs, 'C 33, M 40, LVIS parameters, ties, 2 batches', L.random_images(2, 4, 33, 40, 30, scores_levels=16, gt_classes=4),
                   33, 40, 31, max_dets=(20,), splits=2)
        check_case(libs, 'C 65, no neg list, no nel list', L.random_images(3, 3, 65, 20, 30, n_neg=None, n_nel=None, gt_classes=3), 65, 20,
                   30, max_dets=(5, 20), need=('cut',))
        check_case(libs, 'C 32, Kn 0 (the empty set), min_score 0.25', L.random_images(4, 3, 32, 20, 30, n_neg=0, gt_classes=3), 32, 20, 30,
                   max_dets=(15,), min_score=0.25, Kn=0)
        if not quick:
            check_case(libs, 'C 5, M 257, T 15, neg = all', L.random_images(5, 2, 5, 257, 40, n_neg=5),
                       5, 257, 40, thresholds=np.linspace(0.25, 0.95, 15), max_dets=(30,), need=('cut', 'nel'))
            check_case(libs, 'C 1203, M 16, 300 of 320 slots, cap 300', L.random_images(6, 2, 1203, 16, 320, n_neg=6, n_nel=3, gt_classes=5),
                       1203, 16, 320, splits=2)


if __name__ == '__main__':
    main()
