"""Open-set detection evaluation without a GPU: the numpy restatement (tests/_eval_open_ref.py) against a worked example and
against tests/_eval_scale_ref.py with one more class, the closed-form k_star rule of the kernel against OWOD's brute-force rule,
and the host-side argument checks."""
import ctypes
import os

import numpy as np
import pytest

import _eval_open_ref as O
import _eval_scale_ref as R

LEVELS = (0.8, 0.5, 0.625, 0.1, 1.0)


def _worked_example():
    """C = 2 (0-based: known 0, 1; unknown 2), one image"""
    return dict(gt_boxes=np.array([[0, 0, 10, 10], [20, 20, 30, 30]], np.float32), gt_classes=np.array([0, 2]),
                det_boxes=np.array([[20, 20, 30, 30], [0, 0, 10, 10], [20, 20, 30, 30], [40, 40, 50, 50]], np.float32),
                det_scores=np.array([0.95, 0.9, 0.7, 0.6], np.float32), det_classes=np.array([0, 0, 2, 1]))


def test_restatement_on_the_worked_example():
    r = O.evaluate([_worked_example()], 2, (0.5,), 0.8)
    assert r['flags'].tolist() == [0, 1, 1, 0] and r['open'].tolist() == [1, 0, 0, 0]
    assert r['a_ose'].tolist() == [1]
    assert (r['k_star'][0, 0], r['pos'][0, 0], r['rank_at'][0, 0], r['open_at'][0, 0]) == (1, 1, 2, 1)
    assert r['wi'].tolist() == [0.5]
    assert r['u_recall'].tolist() == [1.0] and r['u_precision'].tolist() == [1.0] and r['u_ap'].tolist() == [1.0]
    assert r['ap'][0, 0] == 0.5 and np.isnan(r['ap'][0, 1])
    assert r['pos'][0, 1] == -1 and r['n_det'][0].tolist() == [2, 1, 1] and r['tp'][0].tolist() == [1, 0, 1]
    assert r['recall'][0, 0] == 1.0 and r['precision'][0, 0] == 0.5 and r['precision_at_recall'][0, 0] == 0.5


def test_restatement_equals_the_closed_set_restatement_with_one_more_class():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'evaluation_scale.npz'))
    thresholds = [float(t) for t in g['thresholds']]
    for tag in ('a', 'b'):
        images, C1 = R.fixture_case(g, tag)                 # the fixture's last class plays the unknown one
        ref = R.evaluate(images, C1, thresholds)
        r = O.evaluate(images, C1 - 1, thresholds, 0.8)
        assert np.array_equal(r['ap'].view(np.int64), ref['ap'].view(np.int64))
        assert np.array_equal(r['flags'], ref['flags'])
        for k in ('gt_count', 'gt_imgs', 'correct'):
            assert np.array_equal(r[k], ref[k])
        order = O.sorted_order(ref['scores'], ref['classes'], ref['flags'], C1)
        for t in range(len(thresholds)):
            for c in range(C1):
                f = ref['flags'][order][ref['classes'][order] == c]
                assert r['n_det'][t, c] == int((((f >> np.uint32(16 + t)) & 1) == 0).sum())
                assert r['tp'][t, c] == int(((f >> np.uint32(t)) & 1).sum())
        assert (r['open_at'] <= r['open_total']).all() and (r['rank_at'] <= r['n_det']).all() and (r['pos'][:, :C1 - 1] >= 0).any()


def test_closed_form_k_star_equals_the_brute_force_rule():
    from ood_object_detection_amd.effdet.evaluation.open_set_evaluator import k_star_closed_form
    rs = np.random.RandomState(5)
    seen_tie = False
    for case in range(4000):
        n_gt = int(rs.randint(1, 41))
        n = int(rs.randint(1, 60))
        tp = (rs.uniform(size=n) < rs.choice([0.0, 0.2, 0.6, 1.0])).astype(int)
        tp[np.nonzero(np.cumsum(tp) > n_gt)[0]] = 0                         # at most n_gt true positives
        ctp = np.cumsum(tp)
        for level in LEVELS:
            pos = O.brute_force_position(ctp, n_gt, level)
            k = k_star_closed_form(level, n_gt, int(ctp[-1]), bool(tp[0]))
            assert k == ctp[pos], (case, level, n_gt, tp.tolist())
            assert pos == int(np.argmax(ctp == k))                           # the first position with that count
            seen_tie |= n_gt == 4 and level == 0.625 and ctp[-1] >= 3 and k == 2
    assert seen_tie                                                          # |2/4 - 0.625| == |3/4 - 0.625|: the smaller count


# ------------------------------------------------------------------------------------------------ host-side argument checks
P = 0x1000                                                                   # a non-null pointer that is never dereferenced


def _lib():
    from ood_object_detection_amd import _lib
    return _lib.load()


def test_host_queries_and_c_abi_argument_checks():
    lib = _lib()
    closed, opened = lib.effdet_eval_ap_sorted_workspace_bytes(1 << 20, 81), lib.effdet_eval_open_sorted_workspace_bytes(1 << 20, 81)
    assert opened - closed >= 2 * 4 * (1 << 20)                              # two more payload buffers
    assert lib.effdet_eval_open_sorted_result_bytes(10, 81) == lib.effdet_eval_ap_sorted_result_bytes(10, 81) + 8 * 7 * 10 * 81
    for bad in ((0, 81), ((1 << 24) + 1, 81), (1000, 0), (1000, 65536)):
        assert lib.effdet_eval_open_sorted_workspace_bytes(*bad) == -22 and lib.effdet_eval_open_sorted_offset(*bad, 0) == -22
    offs = [lib.effdet_eval_open_sorted_offset(1000, 81, w) for w in (0, 1, 2)]
    assert len(set(offs)) == 3 and min(offs) >= 0 and max(offs) + 4000 <= lib.effdet_eval_open_sorted_workspace_bytes(1000, 81)
    assert lib.effdet_eval_open_sorted_offset(1000, 81, 3) == -22
    for bad in ((0, 81), (17, 81), (1, 1), (1, 65536)):
        assert lib.effdet_eval_open_sorted_result_bytes(*bad) == -22
    thr = (ctypes.c_float * 17)(*[0.05 * (i + 1) for i in range(17)])
    words = lambda T=1, C=6, B=2, max_det=10, M=4, det=P, open_=P: \
        lib.effdet_eval_open_words(None, det, P, P, P, B, max_det, M, C, thr, T, open_)
    assert words(T=0) == -22 and words(T=17) == -22 and words(C=1) == -22 and words(C=65536) == -22
    assert words(B=0) == -22 and words(max_det=0) == -22 and words(M=0) == -22 and words(det=None) == -22 and words(open_=None) == -22
    nb = lib.effdet_eval_open_sorted_workspace_bytes(1000, 6)
    srt = lambda level=0.8, T=1, C=6, n=10, open_=P, short=0: \
        lib.effdet_eval_open_sorted(None, P, P, P, open_, 1000, n, P, T, C, P, P, P, level, P, nb - short, P)
    for level in (0.0, -0.5, 1.5, float('nan')):
        assert srt(level=level) == -22
    assert srt(T=17) == -22 and srt(C=65536) == -22 and srt(C=1) == -22 and srt(n=1001) == -22 and srt(open_=None) == -22
    assert srt(short=1) == -22
    app = lambda open_=P, out=P, cap=100: lib.effdet_eval_append_open(None, P, P, open_, P, 2, 10, P, P, P, out, cap, P)
    assert app(open_=None) == -22 and app(out=None) == -22 and app(cap=0) == -22
    rel = lambda C=5, B=2, det=P, pitch=10: lib.effdet_relabel_unknown(None, det, P, P, pitch, 1, B, 10, C, 0.5, None, P)
    assert rel(C=0) == -22 and rel(C=65535) == -22 and rel(B=0) == -22 and rel(det=None) == -22 and rel(pitch=-1) == -22


def test_python_api_argument_checks():
    import torch
    from ood_object_detection_amd import ood
    from ood_object_detection_amd.effdet.evaluation import OpenSetDetectionEvaluator
    cats = [{'id': 1, 'name': 'a'}, {'id': 2, 'name': 'b'}]
    for level in (0.0, 1.5, -1.0, float('nan')):
        with pytest.raises(ValueError):
            OpenSetDetectionEvaluator(cats, recall_level=level)
    with pytest.raises(ValueError):
        OpenSetDetectionEvaluator(cats, iou_thresholds=tuple(0.05 * i for i in range(1, 18)))
    with pytest.raises(ValueError):
        OpenSetDetectionEvaluator([{'id': 65535, 'name': 'a'}])                 # C + 1 > 65535
    with pytest.raises(ValueError):
        OpenSetDetectionEvaluator(cats + [{'id': 3, 'name': 'unknown'}])         # the unknown class is implicit
    with pytest.raises(ValueError):
        OpenSetDetectionEvaluator([{'id': 0, 'name': 'a'}, {'id': 1, 'name': 'b'}])
    with pytest.raises(ValueError):
        OpenSetDetectionEvaluator(cats + [{'id': 2, 'name': 'c'}])               # one id twice
    with pytest.raises(RuntimeError):
        OpenSetDetectionEvaluator(cats, device='cpu')
    det, cnt, sc = torch.zeros(2, 5, 6), torch.zeros(2, dtype=torch.int32), torch.zeros(2, 5)
    with pytest.raises(RuntimeError):
        ood.relabel_unknown(det, cnt, sc, 0.5, 2)                                # CPU tensors: no CPU fallback
