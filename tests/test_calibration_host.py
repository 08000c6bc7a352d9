"""Detection calibration without a GPU: the numpy restatement (tests/_calibration_ref.py) on worked examples computed by hand, its
Newton state machine on Bernoulli data drawn from a known map, the host glue of effdet/evaluation/calibration_evaluator.py
against the restatement, the argument checks of csrc/calibration_eval.hip's C ABI and of the Python classes, the factory, and the
state_dict round trip."""
import ctypes
import math
import os
import re
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _calibration_ref as R  # noqa: E402
from ood_object_detection_amd import _lib  # noqa: E402
from ood_object_detection_amd.effdet.evaluation import calibration_evaluator as CE  # noqa: E402

TP, FP = np.uint32(1), np.uint32(0)
IGNORED = np.uint32(1 << 16)


def _tables(scores, flags, iou=None, classes=None, C=1, T=1, K=2):
    scores = np.asarray(scores, np.float32)
    iou = np.zeros(len(scores), np.float32) if iou is None else np.asarray(iou, np.float32)
    classes = np.zeros(len(scores), np.int64) if classes is None else np.asarray(classes, np.int64)
    return R.tables(scores, classes, np.asarray(flags, np.uint32), iou, C, T, K)


def _both(r, t=0):
    """the restatement's metrics and the product's host glue over the same tables: equal bitwise"""
    a, b = R.metrics(r, t), CE.calibration_metrics(r, t)
    for k in a:
        assert (a[k] == b[k]) or (a[k] != a[k] and b[k] != b[k]), k
    return a


def test_d_ece_worked_example():
    """scores 0.9, 0.8, 0.3, 0.2 with tp 1, 0, 1, 0 and two bins: gaps 0.35 and 0.25, D-ECE 0.30.  The scores are float32, each
    within 2^-25 of its decimal, so the figures are compared with the decimals at 2^-24 and with the exact rational value of the
    float32 inputs at a few float64 roundings"""
    s = np.array([0.9, 0.8, 0.3, 0.2], np.float32)
    r = _tables(s, [TP, FP, TP, FP])
    assert r['bins']['n'][0, 1, 0].tolist() == [2, 2] and r['bins']['tp'][0, 1, 0].tolist() == [1, 1]
    _, _, gaps = CE.bin_gaps(r['bins']['n'][0, 1, 0], r['bins']['sum_p'][0, 1, 0], r['bins']['tp'][0, 1, 0])
    assert abs(gaps[1] - 0.35) <= 2.0 ** -24 and abs(gaps[0] - 0.25) <= 2.0 ** -24
    m = _both(r)
    assert abs(m['D-ECE'] - 0.30) <= 2.0 ** -24 and abs(m['MCE'] - 0.35) <= 2.0 ** -24
    f = [Fraction(float(v)) for v in s]
    exact = Fraction(1, 2) * abs((f[0] + f[1]) / 2 - Fraction(1, 2)) + Fraction(1, 2) * abs((f[2] + f[3]) / 2 - Fraction(1, 2))
    assert abs(m['D-ECE'] - float(exact)) <= 8 * 2.0 ** -53
    assert m['ACE'] == m['D-ECE']                                             # four entries, two bins: the same partition
    assert m['classwise-ECE'] == m['D-ECE']                                   # one class
    brier = (0.1 ** 2 + 0.8 ** 2 + 0.7 ** 2 + 0.2 ** 2) / 4
    assert abs(m['Brier'] - brier) <= 2.0 ** -22
    nll = -(math.log(0.9) + math.log(0.2) + math.log(0.3) + math.log(0.8)) / 4
    assert abs(m['NLL'] - nll) <= 2.0 ** -20


def test_laece_worked_example():
    """one class, two bins; 0.75 (true positive, IoU 0.5) and 0.25 (true positive, IoU 1.0): LaECE = 0.5 |0.75 - 0.5| + 0.5 |0.25 - 1|
    = 0.5, all dyadic, so exact; the confidence-only D-ECE of the same table is 0.5 |0.75 - 1| + 0.5 |0.25 - 1| = 0.5 too"""
    r = _tables([0.75, 0.25], [TP, TP], iou=[0.5, 1.0])
    m = _both(r)
    assert m['LaECE'] == 0.5 and m['D-ECE'] == 0.5
    assert r['bins']['sum_iou'][0, 0, 0].tolist() == [1.0, 0.5]
    d = CE.reliability_diagram(r, 0)
    assert d['confidence'].tolist() == [0.25, 0.75] and d['precision'].tolist() == [1.0, 1.0] and d['iou'].tolist() == [1.0, 0.5]


def test_ignored_entry_keeps_its_mass_position():
    """0.9 tp, 0.8 ignored (matched a difficult box), 0.7 fp, 0.6 tp; two mass bins of m = 4: positions [0, 2) and [2, 4).  The ignored
    entry adds to no n, in neither scheme, but keeps position 1: the mass bins hold 1 and 2 entries, not 2 and 1"""
    r = _tables([0.9, 0.8, 0.7, 0.6], [TP, IGNORED, FP, TP])
    b = r['bins']
    assert b['n'][0, 1, 1].tolist() == [1, 2] and b['tp'][0, 1, 1].tolist() == [1, 1]
    assert b['n'][0, 1, 0].tolist() == [0, 3] and int(r['entries'][0, 1]) == 4
    assert b['sum_p'][0, 1, 1, 0] == float(np.float32(0.9))
    _both(r)


def test_edges_empty_bins_and_score_one():
    """K = 4: 0.5 lies exactly on an edge and belongs to bin 2, 1.0 to bin K - 1 = 3, 0.0 to bin 0, bin 1 stays empty and adds
    nothing; a score above 1 is clamped into the last bin and counted out of range"""
    r = _tables([1.0, 0.5, 0.0], [TP, FP, FP], K=4)
    assert r['bins']['n'][0, 1, 0].tolist() == [1, 0, 1, 1]
    m = _both(r)
    assert m['D-ECE'] == (1.0 / 3) * 0.0 + (1.0 / 3) * 0.5 + (1.0 / 3) * 0.0
    assert int(r['out_of_range'][0, 1]) == 0
    r = _tables([1.5, 0.5], [TP, FP], K=4)
    assert r['bins']['n'][0, 1, 0].tolist() == [0, 0, 1, 1] and int(r['out_of_range'][0, 1]) == 1
    assert R.width_bin(np.float32(0.99999994), 64) == 63 and R.width_bin(np.float32(-0.25), 8) == 0
    r = _tables([], [], K=3)
    assert all(v != v for k, v in _both(r).items())                           # no entries: every metric is NaN


def test_score_threshold_applies_after_matching():
    """two detections on one box: 0.9 takes it; 0.2 (IoU 1 with the same box) is a false positive, and with score_threshold 0.5 it is
    matched all the same and then left out; with the detections' roles swapped the low one still takes the box"""
    box = np.array([[0, 0, 10, 10]], np.float32)
    im = dict(gt_boxes=box, gt_classes=np.array([0]), det_boxes=np.concatenate([box, box]), det_scores=np.array([0.9, 0.2], np.float32),
              det_classes=np.array([0, 0]))
    acc = R.accumulate([im], 1, [0.5], 0.5)
    assert acc['per_image'][0][0].tolist() == [1, 0] and acc['per_image'][0][1].tolist() == [1.0, 1.0]
    assert acc['scores'].tolist() == [np.float32(0.9)] and acc['flags'].tolist() == [1]
    im2 = dict(im, det_scores=np.array([0.4, 0.2], np.float32))
    acc = R.accumulate([im2], 1, [0.5], 0.3)
    assert acc['per_image'][0][0].tolist() == [1, 0] and acc['scores'].tolist() == [np.float32(0.4)]
    acc = R.accumulate([im2], 1, [0.5], 0.5)
    assert acc['per_image'][0][0].tolist() == [1, 0] and len(acc['scores']) == 0 and acc['gt_count'].tolist() == [1]


def test_matching_agrees_with_the_ap_units():
    """the flag words are those of tests/_eval_scale_ref.py (asserted by construction) and the candidate IoU is the largest of the
    class, 0 for a class without a box and for dropped detections"""
    import _eval_openimages_ref as O
    images = O.dense_case(3, 2, 4, 40, 50, 0.0)
    for im in images:
        f, u, _ = R.match_image(im, 4, [0.5, 0.75])
        assert ((u == 0) | ((f & R.INVALID) == 0)).all()
        hit = (f & np.uint32(0x00030003)) != 0
        assert (u[hit] >= np.float32(0.5)).all() and (u <= 1).all()


@pytest.mark.parametrize('case', range(len(R.FIT_CASES)))
def test_newton_restatement_recovers_the_map(case):
    """Bernoulli labels drawn from sigmoid(a0 logit(p) + b0): the state machine converges from (1, 0) with ZERO halvings, to the
    same point for sequential and pairwise summation, near (a0, b0), and the gradient there is rounding.  Gradient bound: the
    last direction d is <= 2^-40 max(1, |a|, |b|) and g = H d with H_aa <= n x_max^2 / 4, H_ab <= n x_max / 4, x_max = logit(1 - 2^-24)"""
    n, a0, b0 = R.FIT_CASES[case]
    s, f, u = R.bernoulli_case(100 + case, n, a0, b0)
    x, y = R.fit_data(s, f, u, 0, 'tp')
    r = R.newton_fit(x, y, 'platt', summation='pairwise')
    q = R.newton_fit(x, y, 'platt', summation='sequential')
    assert r['converged'] and r['halvings'] == 0 and 5 <= r['iterations'] <= 11, r
    assert q['converged'] and q['halvings'] == 0 and q['iterations'] == r['iterations']
    assert abs(r['a'] - q['a']) <= 1e-15 * max(1.0, abs(r['a'])) and abs(r['b'] - q['b']) <= 1e-15 * max(1.0, abs(r['b']))
    se = 6.0 / math.sqrt(n)                                                   # a generous sampling error of the estimate
    assert abs(r['a'] - a0) <= se * max(1.0, a0) * 4 and abs(r['b'] - b0) <= se * 4, r
    xmax = float(R.logit(1.0))
    bound = n * 0.25 * (xmax * xmax + xmax) * 2.0 ** -40 * max(1.0, abs(r['a']), abs(r['b']))
    assert max(abs(g) for g in r['gradient']) <= bound, (r['gradient'], bound)
    assert r['nll_after'] <= r['nll_before']
    for target, method in (('iou', 'platt'), ('tp', 'temperature'), ('iou', 'temperature')):
        x, y = R.fit_data(s, f, u, 0, target)
        t = R.newton_fit(x, y, method)
        assert t['converged'] and t['halvings'] == 0 and t['a'] > 0, (target, method, t)
        assert method == 'platt' or t['b'] == 0.0


def test_newton_restatement_constant_target_does_not_converge():
    """every target equal: the data are separable, b runs away; the machine ends as "not converged" with finite numbers"""
    s, f, u = R.bernoulli_case(7, 500, 1.0, 0.0)
    x, y = R.fit_data(s, np.ones_like(f), u, 0, 'tp')
    for method in ('platt', 'temperature'):
        # temperature has no offset: a constant target is separable for it only when every logit has the same sign
        r = R.newton_fit(x if method == 'platt' else np.abs(x) + 0.125, y, method)
        assert not r['converged'] and math.isfinite(r['a']) and math.isfinite(r['b']) and math.isfinite(r['nll_after']), r
    r = R.newton_fit(np.zeros(0), np.zeros(0))                                # no entries
    assert not r['converged'] and (r['a'], r['b']) == (1.0, 0.0)


def test_apply_restatement_is_monotone_and_clamped():
    p = np.sort(np.random.RandomState(3).uniform(0, 1, 4000).astype(np.float32))[::-1]
    p[:3], p[-3:] = 1.0, 0.0
    for a, b in ((1.5, -0.5), (0.05, 2.0), (8.0, 0.0)):
        q = R.apply_scores(p, a, b)
        assert q.dtype == np.float32 and (np.diff(q) <= 0).all() and (q >= 0).all() and (q <= 1).all()
    assert np.array_equal(R.apply_scores(p, 1.0, 0.0)[5:-5], p[5:-5])         # the identity map, away from the clamp
    det = np.zeros((2, 5, 6), np.float32)
    det[..., 4] = 0.5
    out = R.apply_det(det, [2, 9], 2.0, 1.0)
    assert (out[0, 2:, 4] == 0.5).all() and (out[0, :2, 4] != 0.5).all() and (out[1, :, 4] != 0.5).all()


def test_argument_checks_of_the_classes():
    import torch
    from ood_object_detection_amd.calibration import DetectionCalibrator
    from ood_object_detection_amd.effdet.evaluation import CalibrationEvaluator
    cats = [dict(id=i + 1, name=str(i)) for i in range(3)]
    for kw in (dict(bins=0), dict(bins=65), dict(iou_thresholds=[0.5] * 17), dict(iou_thresholds=[0.75, 0.5]), dict(iou_thresholds=[]),
               dict(score_threshold=float('nan')), dict(capacity=0)):
        with pytest.raises(ValueError):
            CalibrationEvaluator(cats, **kw)
    many = [dict(id=i + 1, name=str(i)) for i in range(1024)]
    with pytest.raises(ValueError):
        CalibrationEvaluator(many, iou_thresholds=np.linspace(0.5, 0.95, 16), bins=64)      # 16 * 1025 * 64 > 2^20
    with pytest.raises(RuntimeError):
        CalibrationEvaluator(cats, device='cpu')
    with pytest.raises(ValueError):
        DetectionCalibrator(method='isotonic')
    with pytest.raises(ValueError):
        DetectionCalibrator(target='box')
    with pytest.raises(RuntimeError):
        DetectionCalibrator(device='cpu')
    cal = DetectionCalibrator()
    with pytest.raises(RuntimeError):
        cal.apply(torch.zeros(1, 4, 6), torch.zeros(1, dtype=torch.int32))    # CPU tensors: no fallback
    with pytest.raises(RuntimeError):
        cal.state_dict()                                                      # nothing fitted


def test_argument_checks_of_the_c_abi():
    """refused before anything is launched: callable without a GPU"""
    lib = _lib.load()
    assert lib.effdet_calibration_result_bytes(1, 1, 1) == 8 * (8 + 8 * 2 + 4 * 2 + 2 + 1)
    assert lib.effdet_calibration_result_bytes(16, 90, 64) == 8 * (8 + 8 * 16 * 91 * 64 + 4 * 16 * 91 + 180 + 16 * 90)
    for T, C, K in ((0, 1, 1), (17, 1, 1), (1, 0, 1), (1, 65536, 1), (1, 1, 0), (1, 1, 65), (16, 1024, 64)):
        assert lib.effdet_calibration_result_bytes(T, C, K) <= 0, (T, C, K)
    assert lib.effdet_calibration_result_bytes(16, 1023, 64) > 0
    assert lib.effdet_calibration_workspace_bytes(1 << 24, 90) > 0 and lib.effdet_calibration_workspace_bytes((1 << 24) + 1, 90) <= 0
    assert lib.effdet_calibration_workspace_bytes(0, 90) <= 0 and lib.effdet_calibration_sorted_offset(100, 3, 6) <= 0
    offs = [lib.effdet_calibration_sorted_offset(5000, 3, w) for w in range(6)]
    assert len(set(offs)) == 6 and all(0 <= o < lib.effdet_calibration_workspace_bytes(5000, 3) for o in offs)
    assert lib.effdet_calibration_fit_workspace_bytes(2048) == 64 and lib.effdet_calibration_fit_workspace_bytes(2049) == 128
    assert lib.effdet_calibration_fit_workspace_bytes(0) <= 0
    buf = np.zeros(64, np.float64)
    p = buf.ctypes.data
    thr = (ctypes.c_float * 2)(0.5, 0.75)
    bad = (ctypes.c_float * 2)(0.75, 0.5)
    match = lambda **k: lib.effdet_calibration_match(None, p, p, p, p, None, k.get('B', 1), k.get('max_det', 4), k.get('M', 2), k.get('C', 3),
                                                     k.get('thr', thr), k.get('T', 2), k.get('st', 0.0), p, k.get('iou', p), p, p, p, p)
    for k in (dict(B=0), dict(max_det=0), dict(M=0), dict(C=0), dict(thr=bad), dict(T=17), dict(st=float('nan')), dict(iou=None),
              dict(M=6000)):
        assert match(**k) == -22, k
    assert lib.effdet_calibration_append(None, p, p, p, p, 1, 4, 0.0, p, p, p, None, 16, p) == -22
    assert lib.effdet_calibration_append(None, p, p, p, p, 1, 4, 0.0, p, p, p, p, 0, p) == -22
    assert lib.effdet_calibration_table(None, p, p, p, p, 16, -1, p, 1, 3, 65, p, p, p, p, 1 << 20, p) == -22
    assert lib.effdet_calibration_table(None, p, p, p, p, 16, -1, None, 1, 3, 15, p, p, p, p, 1 << 20, p) == -22
    assert lib.effdet_calibration_table(None, p, p, p, p, 16, 17, p, 1, 3, 15, p, p, p, p, 1 << 20, p) == -22
    assert lib.effdet_calibration_table(None, p, p, p, p, 16, -1, p, 1, 3, 15, p, p, p, p, 8, p) == -22
    assert lib.effdet_calibration_fit_step(None, p, p, p, 16, p, 16, 0, 0, p, p, 64) == -22
    assert lib.effdet_calibration_fit_step(None, p, p, p, 4096, p, 0, 0, 0, p, p, 64) == -22
    assert lib.effdet_calibration_fit_step(None, p, p, p, 16, p, 0, 0, 0, None, p, 64) == -22
    assert lib.effdet_calibration_apply(None, p, p, p, 0, 4, p) == -22 and lib.effdet_calibration_apply(None, p, p, None, 1, 4, p) == -22


def test_header_declares_the_entry_points():
    header = open(os.path.join(ROOT, 'include', 'effdet_hip.h')).read()
    declared = set(re.findall(r'\b(effdet_calibration_[a-z0-9_]+)\s*\(', header))
    assert declared == {n for n in _lib.SIGNATURES if n.startswith('effdet_calibration_')} and len(declared) == 9
    for name in declared:
        proto = re.search(r'\b%s\s*\(([^;]*)\);' % name, header).group(1)
        assert len(proto.split(',')) == len(_lib.SIGNATURES[name][1]), name
    mk = open(os.path.join(_lib.CSRC, 'Makefile')).read()
    assert 'build/calibration_eval.o' in mk and re.search(r'^EXTRA_calibration_eval = -ffp-contract=off$', mk, re.M)


class _Parser:
    img_ids = [7]
    cat_dicts = [dict(id=1, name='a'), dict(id=2, name='b')]


class _Dataset:
    parser = _Parser()


def test_create_evaluator_dispatch():
    from ood_object_detection_amd.effdet import evaluator as E
    ev = E.create_evaluator('calibration', _Dataset(), pred_yxyx=True, bins=10)
    assert type(ev) is E.CalibrationEvaluator and ev.pred_yxyx and not ev.distributed
    assert isinstance(E.CalibrationEvaluator.device_evaluator, property)      # what DetectionCalibrator.fit takes from the wrapper
    assert type(E.create_evaluator('voc2007', _Dataset())) is E.PascalEvaluator           # the other names are unchanged
    assert type(E.create_evaluator('openimages-v5', _Dataset())) is E.OpenImagesEvaluator


def test_state_dict_round_trip():
    from ood_object_detection_amd.calibration import DetectionCalibrator
    cal = DetectionCalibrator().load_state_dict(dict(a=1.75, b=-0.25, method='temperature', target='iou'))
    sd = cal.state_dict()
    assert sd == dict(a=1.75, b=-0.25, method='temperature', target='iou') and cal.method == 'temperature' and cal.target == 'iou'
    assert DetectionCalibrator().load_state_dict(sd).state_dict() == sd
    assert cal.finish()['converged'] and cal.finish()['a'] == 1.75
    for bad in (dict(sd, a=0.0), dict(sd, a=-1.0), dict(sd, b=float('nan')), dict(sd, method='isotonic'), dict(sd, a=float('inf'))):
        with pytest.raises(ValueError):
            DetectionCalibrator().load_state_dict(bad)


def test_d_ece_against_netcal():
    """only where netcal happens to be installed: its confidence-only ECE on the worked example"""
    netcal = pytest.importorskip('netcal.metrics')
    s = np.array([0.9, 0.8, 0.3, 0.2], np.float32)
    y = np.array([1, 0, 1, 0])
    r = _tables(s, [TP, FP, TP, FP])
    got = netcal.ECE(2, detection=True).measure(s.astype(np.float64)[:, None], y)
    assert abs(got - R.metrics(r, 0)['D-ECE']) <= 1e-12
