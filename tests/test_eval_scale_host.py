"""Dataset-scale detection evaluation without a GPU: the numpy restatement (tests/_eval_scale_ref.py) against the reference's own
evaluator (tests/golden/evaluation_scale.npz: `difficult` ground truth, IoU thresholds 0.5 / 0.55 / 0.75) and against
oracle/evaluation.py, and the host-side argument checks of csrc/eval_scale.hip."""
import ctypes

import numpy as np
import pytest

import _eval_scale_ref as R
from _seeded import eval_case, eval_case_dense
from oracle import evaluation as oe


def _golden():
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'evaluation_scale.npz'))


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_restatement_equals_the_reference_evaluator(tag):
    g = _golden()
    images, C = R.fixture_case(g, tag)
    thresholds = [float(t) for t in g['thresholds']]
    assert thresholds == [0.5, 0.55, 0.75]
    r = R.evaluate(images, C, thresholds)
    for t in range(len(thresholds)):
        assert np.allclose(r['ap'][t], g[tag + '_ap'][t], rtol=0, atol=1e-12, equal_nan=True), (tag, t)
        assert np.array_equal(np.isnan(r['ap'][t]), np.isnan(g[tag + '_ap'][t]))
        assert np.allclose(r['corloc'][t], g[tag + '_cl'][t], rtol=0, atol=1e-12, equal_nan=True), (tag, t)
        assert np.array_equal(np.isnan(r['corloc'][t]), np.isnan(g[tag + '_cl'][t]))
        assert abs(r['mean_ap'][t] - g[tag + '_map'][t]) <= 1e-12 and abs(r['mean_corloc'][t] - g[tag + '_corloc'][t]) <= 1e-12
        inside = (g[tag + '_ap'][t] > 0) & (g[tag + '_ap'][t] < 1)
        assert inside.sum() >= 2                                            # the fixture discriminates at every threshold
    assert g[tag + '_difficult'].sum() > 0


def test_fixture_differs_from_the_evaluation_without_difficult_flags():
    g = _golden()
    images, C = R.fixture_case(g, 'a')
    plain = R.evaluate([{k: v for k, v in im.items() if k != 'gt_difficult'} for im in images], C, [0.5])
    assert not np.allclose(plain['ap'][0], g['a_ap'][0], rtol=0, atol=1e-6, equal_nan=True)


@pytest.mark.parametrize('thr', [0.5, 0.75])
def test_restatement_without_flags_equals_the_oracle(thr):
    cases = [(eval_case(31, 10, 6, 40), 6), (eval_case(32, 3, 20, 100), 20), (eval_case_dense(7, 3, 5, 70, 60, cls=2), 5)]
    for images, C in cases:
        z = [R.zero_based(im) for im in images]
        with np.errstate(all='ignore'):
            o = oe.evaluate(z, C, thr)
            r = R.evaluate(z, C, [thr])
        assert np.array_equal(r['ap'][0], o['per_class_ap'], equal_nan=True)
        assert np.array_equal(r['corloc'][0], o['per_class_corloc'], equal_nan=True)
        assert r['mean_ap'][0] == o['mean_ap'] and r['mean_corloc'][0] == o['mean_corloc']
        # all-false difficult flags change nothing
        r2 = R.evaluate([dict(im, gt_difficult=np.zeros(len(im['gt_classes']), bool)) for im in z], C, [thr])
        assert np.array_equal(r2['flags'], r['flags']) and np.array_equal(r2['ap'], r['ap'], equal_nan=True)


def test_ignored_detections_and_difficult_ground_truth_in_the_restatement():
    """one class, ground truth A (difficult) and B: a detection on A is ignored, B's detection is the only ranked one -> AP 1 over
    ONE instance; without the flag the duplicate detection of A is a false positive in between"""
    gt = np.array([[0, 0, 10, 10], [30, 30, 40, 40]], np.float32)
    det = np.array([[0, 0, 10, 10], [0, 0, 10, 10], [30, 30, 40, 40]], np.float32)
    im = dict(gt_boxes=gt, gt_classes=np.array([0, 0]), det_boxes=det, det_scores=np.array([0.9, 0.8, 0.7], np.float32),
              det_classes=np.array([0, 0, 0]), gt_difficult=np.array([True, False]))
    r = R.evaluate([im], 1, [0.5, 0.75])
    assert r['flags'].tolist() == [0x30000, 0x30000, 0x3] and r['gt_count'].tolist() == [1] and r['gt_imgs'].tolist() == [1]
    assert r['ap'][:, 0].tolist() == [1.0, 1.0] and r['correct'][:, 0].tolist() == [1, 1]
    im.pop('gt_difficult')
    r = R.evaluate([im], 1, [0.5])
    assert r['flags'].tolist() == [1, 0, 1] and abs(r['ap'][0, 0] - (0.5 + 0.5 * 2 / 3)) < 1e-15


# ------------------------------------------------------------------------------------------------ host-side argument checks
P = 0x1000                                                                   # a non-null pointer that is never dereferenced


def _lib():
    from ood_object_detection_amd import _lib
    return _lib.load()


def test_host_queries():
    lib = _lib()
    tile = lib.effdet_eval_scale_sort_tile()
    assert tile > 0 and tile % 256 == 0
    small, large = lib.effdet_eval_ap_sorted_workspace_bytes(1000, 80), lib.effdet_eval_ap_sorted_workspace_bytes(1 << 20, 80)
    assert 0 < small < large and large - small >= 2 * 12 * ((1 << 20) - 1000)        # two (key, flag word) buffers
    for bad in ((0, 80), ((1 << 24) + 1, 80), (1000, 0), (1000, 65536)):
        assert lib.effdet_eval_ap_sorted_workspace_bytes(*bad) == -22
        assert lib.effdet_eval_ap_sorted_offset(*bad, 0) == -22
    assert lib.effdet_eval_ap_sorted_workspace_bytes(1 << 24, 65535) > 0
    for C in (80, 255, 256, 65535):
        k, f = (lib.effdet_eval_ap_sorted_offset(1000, C, w) for w in (0, 1))
        assert k >= 0 and f >= 0 and k % 8 == 0 and abs(k - f) >= 4000 and max(k + 8000, f + 4000) <= lib.effdet_eval_ap_sorted_workspace_bytes(1000, C)
    assert lib.effdet_eval_ap_sorted_offset(1000, 80, 2) == -22
    assert lib.effdet_eval_ap_sorted_result_bytes(10, 80) == 8 * (8 + 2 * 10 * 80 + 2 * 80)
    for bad in ((0, 80), (17, 80), (1, 0), (1, 65536)):
        assert lib.effdet_eval_ap_sorted_result_bytes(*bad) == -22


def _match_multi(lib, thr, T=None, C=5, det=P, cnt=P, gtb=P, gtc=P, flags=P, g0=P, g1=P, g2=P, B=2, max_det=10, M=4):
    arr = (ctypes.c_float * max(len(thr), 1))(*thr)
    return lib.effdet_eval_match_multi(None, det, cnt, gtb, gtc, None, B, max_det, M, C, arr, len(thr) if T is None else T,
                                       flags, None, g0, g1, g2)


def test_match_multi_argument_checks():
    lib = _lib()
    assert _match_multi(lib, []) == -22 and _match_multi(lib, [0.5] * 16, T=17) == -22                  # T out of range
    assert _match_multi(lib, [0.5, 0.5]) == -22 and _match_multi(lib, [0.75, 0.5]) == -22              # not ascending
    assert _match_multi(lib, [0.5, float('nan')]) == -22
    for name in ('det', 'cnt', 'gtb', 'gtc', 'flags', 'g0', 'g1', 'g2'):                              # null pointers
        assert _match_multi(lib, [0.5], **{name: None}) == -22, name
    assert lib.effdet_eval_match_multi(None, P, P, P, P, None, 2, 10, 4, 5, None, 1, P, None, P, P, P) == -22
    assert _match_multi(lib, [0.5], C=0) == -22 and _match_multi(lib, [0.5], C=65536) == -22            # C out of range
    assert _match_multi(lib, [0.5], B=0) == -22 and _match_multi(lib, [0.5], max_det=0) == -22 and _match_multi(lib, [0.5], M=0) == -22
    assert _match_multi(lib, [0.5], M=6000) == -22                                                      # LDS
    assert _match_multi(lib, [0.5], B=1 << 20, max_det=17) == -22                                       # B * max_det > 2^24


def _ap_sorted(lib, capacity=1000, n=10, T=1, C=5, short=0, state=P, **null):
    p = dict(scores=P, classes=P, flags=P, g0=P, g1=P, g2=P, ws=P, res=P)
    p.update(null)
    nb = lib.effdet_eval_ap_sorted_workspace_bytes(capacity, C)
    return lib.effdet_eval_ap_sorted(None, p['scores'], p['classes'], p['flags'], capacity, n, state, T, C, p['g0'], p['g1'], p['g2'],
                                     p['ws'], (nb if nb > 0 else 1 << 20) - short, p['res'])


def test_ap_sorted_argument_checks():
    lib = _lib()
    assert _ap_sorted(lib, T=0) == -22 and _ap_sorted(lib, T=17) == -22                                 # T out of range
    assert _ap_sorted(lib, C=0) == -22 and _ap_sorted(lib, C=65536) == -22                              # C out of range
    assert _ap_sorted(lib, n=1001) == -22                                                               # n above the capacity
    assert _ap_sorted(lib, capacity=0, n=0) == -22 and _ap_sorted(lib, capacity=(1 << 24) + 1) == -22
    assert _ap_sorted(lib, short=1) == -22                                                              # workspace too small
    for name in ('scores', 'classes', 'flags', 'g0', 'g1', 'g2', 'ws', 'res'):                        # null pointers
        assert _ap_sorted(lib, **{name: None}) == -22, name
    assert _ap_sorted(lib, n=-1, state=None) == -22                                                     # device count without a cursor
    assert _ap_sorted(lib, ws=P + 4) == -22                                                             # alignment


def test_append_argument_checks():
    lib = _lib()
    call = lambda det=P, flags=P, kept=P, B=2, max_det=10, s=P, c=P, f=P, cap=100, st=P: \
        lib.effdet_eval_append(None, det, flags, kept, B, max_det, s, c, f, cap, st)
    for name in ('det', 'flags', 'kept', 's', 'c', 'f', 'st'):
        assert call(**{name: None}) == -22, name
    assert call(B=0) == -22 and call(max_det=0) == -22 and call(cap=0) == -22 and call(cap=(1 << 24) + 1) == -22


def test_python_api_argument_checks():
    from ood_object_detection_amd.effdet.evaluation import DatasetDetectionEvaluator, ObjectDetectionEvaluator
    cats = [{'id': 1, 'name': 'a'}]
    with pytest.raises(RuntimeError):
        DatasetDetectionEvaluator(cats, device='cpu')
    for bad in ((), (0.5, 0.5), (0.75, 0.5), tuple(0.05 * i for i in range(1, 18))):
        with pytest.raises(ValueError):
            DatasetDetectionEvaluator(cats, iou_thresholds=bad)
    for cap in (0, (1 << 24) + 1):
        with pytest.raises(ValueError):
            DatasetDetectionEvaluator(cats, capacity=cap)
    with pytest.raises(ValueError):
        ObjectDetectionEvaluator(cats, ap_method='fast')
