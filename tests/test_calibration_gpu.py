"""csrc/calibration_eval.hip on the device (-m gpu): the matching with the candidate IoU, the append, both sorts, the reliability
tables, the Newton fit and the apply launch, against tests/_calibration_ref.py, against DatasetDetectionEvaluator (flag words and
counters) and against themselves (runs, splits, captured graphs).

Flag words, IoU, counters, n, tp and the mass-bin boundaries are compared EXACTLY.  A float64 sum of n terms >= 0 lies within
n 2^-52 relative of the restatement's correctly rounded sum: each of at most n additions errs by half an ulp of a partial sum that
is no larger than the total.  The fitted (a, b): see FIT_TOL.  Calibrated scores: one float32 ulp (the float64 value is rounded
once, so only a rounding boundary can differ)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _calibration_ref as R
import _eval_openimages_ref as O

DEV = 'cuda:0'
INVALID = 0x80000000
# (a, b) of the device fit against the restatement.  Measured on the data sets of R.FIT_CASES, both targets, both methods: the
# restatement with sequential against pairwise summation differs by at most 2.3e-16, the device from the (pairwise) restatement
# by at most 2.3e-16 as well (0 in seventeen of the twenty runs); the tolerance is 16 times the larger, room for
# the device's log / exp differing by an ulp.
FIT_MEASURED = 2.3e-16
FIT_TOL = 16 * FIT_MEASURED


def _cats(C):
    return [{'id': i + 1, 'name': 'c%d' % i} for i in range(C)]


def _evaluator(C, thresholds=(0.5,), bins=15, **kw):
    from ood_object_detection_amd.effdet.evaluation import CalibrationEvaluator
    return CalibrationEvaluator(_cats(C), iou_thresholds=thresholds, bins=bins, device=DEV, **kw)


def _pack(images, max_det, M):
    det, cnt, gtb, gtc, gtd = O.pack(images, max_det, M)[:5]
    return tuple(torch.from_numpy(a).to(DEV) for a in (det, cnt, gtb, gtc, gtd))


def _u32(t):
    return (t.cpu().numpy().astype(np.int64) & 0xFFFFFFFF).astype(np.uint32)


def _close(got, ref, n):
    got, ref, n = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(n, np.float64)
    err = np.abs(got - ref)
    assert (err <= n * 2.0 ** -52 * np.abs(ref)).all(), float((err / np.maximum(np.abs(ref), 1e-300)).max())


def _compare_tables(got, ref, n_total):
    for k in ('n', 'tp'):
        assert np.array_equal(got['bins'][k], ref['bins'][k]), k
    assert np.array_equal(got['out_of_range'], ref['out_of_range']) and np.array_equal(got['entries'], ref['entries'])
    for k in ('sum_p', 'sum_iou'):
        _close(got['bins'][k], ref['bins'][k], np.maximum(got['bins']['n'], 1))
    terms = np.maximum(got['bins']['n'][:, :, 0].sum(-1), 1)                  # [T, C + 1]: the scope's entries not ignored at t
    assert int(terms.max()) <= max(n_total, 1)
    for k in ('brier', 'nll'):
        _close(got[k], ref[k], terms)


def _fill(ev, scores, classes, flags, iou):
    """entries put into the evaluator's buffers directly, as `add_batch` would have appended them"""
    n = len(scores)
    s, c, f, u, state = ev.entries()
    s[:n].copy_(torch.from_numpy(np.asarray(scores, np.float32)))
    c[:n].copy_(torch.from_numpy(np.asarray(classes, np.int32)))
    f[:n].copy_(torch.from_numpy(np.asarray(flags, np.uint32).view(np.int32)))
    u[:n].copy_(torch.from_numpy(np.asarray(iou, np.float32)))
    state.copy_(torch.tensor([n, 0, 0, 0], dtype=torch.int32))


# ------------------------------------------------------------------------------------------------ matching
MATCH_CASES = [(1, 1), (40, 1), (40, 16), (300, 16), (300, 1)]


@pytest.mark.parametrize('M,T', MATCH_CASES, ids=['M%d-T%d' % c for c in MATCH_CASES])
def test_match_equals_the_ap_unit_and_iou_is_exact(M, T):
    from ood_object_detection_amd.effdet.evaluation import DatasetDetectionEvaluator
    C, n_img, n_det = 5, 3, 60
    thresholds = [0.5] if T == 1 else list(np.linspace(0.2, 0.95, 16))
    images = O.dense_case(700 + M + T, n_img, C, M, n_det, 0.0, classes_used=min(2, M), difficult_frac=0.25)
    args = _pack(images, n_det + 3, M)
    ev = _evaluator(C, thresholds)
    base = DatasetDetectionEvaluator(_cats(C), iou_thresholds=thresholds, device=DEV)
    flags = ev.add_batch(*args)
    assert torch.equal(flags, base.add_batch(*args)) and torch.equal(ev._counters, base._counters)
    iou = ev._last_iou.cpu().numpy()
    flags = _u32(flags)
    thr32 = np.asarray(thresholds, np.float32)
    on_threshold = ties = no_box = ignored = 0
    for i, im in enumerate(images):
        n = len(im['det_scores'])
        rf, ru, _ = R.match_image(im, C, thresholds)
        assert np.array_equal(flags[i, :n], rf) and (flags[i, n:] == INVALID).all()
        assert np.array_equal(iou[i, :n].view(np.uint32), ru.view(np.uint32)) and (iou[i, n:] == 0).all()
        valid = (rf & R.INVALID) == 0
        on_threshold += int(np.isin(ru[valid], thr32).sum())
        ignored += int(((rf[valid] >> 16) != 0).sum())
        no_box += int((valid & ~np.isin(np.asarray(im['det_classes']), np.asarray(im['gt_classes']))).sum())
        gb = np.asarray(im['gt_boxes'])
        ties += int((np.abs(np.diff(gb, axis=0)).sum(1) == 0).sum())
    assert on_threshold > 0 and no_box > 0 and (M == 1 or (ties > 0 and ignored > 0))


# ------------------------------------------------------------------------------------------------ tables
def _entries_case(counts, T, seed, ties=50, ignore=True):
    rs = np.random.RandomState(seed)
    C, n = len(counts), int(sum(counts))
    classes = rs.permutation(np.repeat(np.arange(C), counts)).astype(np.int32)
    scores = (rs.randint(0, ties + 1, n) / float(ties)).astype(np.float32)
    tp = rs.randint(0, 1 << T, n).astype(np.uint32)
    ig = rs.randint(0, 1 << T, n).astype(np.uint32) & rs.randint(0, 1 << T, n).astype(np.uint32) & ~tp & np.uint32(0x7FFF)
    flags = tp | ((ig if ignore else np.zeros_like(ig)) << np.uint32(16))
    return scores, classes, flags, rs.uniform(0, 1, n).astype(np.float32)


_rs = np.random.RandomState(5)
TABLE_CASES = {
    # per-class entry counts around EV_AP_CHUNK = 2048 and RS_TILE = 4096
    'C7-K15-T2-chunks': ([1, 2047, 2048, 2049, 4095, 4096, 4097], 2, 15, 50),
    'C1-K1-T1': ([300], 1, 1, 50),
    'C3-K64-T16': ([100, 0, 3000], 16, 64, 997),
    # one class of 70 000 entries on 41 distinct scores among 90 classes
    'C90-K15-T1-70000': ([70000 if c == 17 else int(v) for c, v in enumerate(_rs.randint(0, 60, 90))], 1, 15, 40),
}
_TABLE_REF = {}


def _table_ref(name):
    if name not in _TABLE_REF:
        counts, T, K, ties = TABLE_CASES[name]
        e = _entries_case(counts, T, 40 + len(counts), ties)
        _TABLE_REF[name] = (e, R.tables(e[0], e[1].astype(np.int64), e[2], e[3], len(counts), T, K))
    return _TABLE_REF[name]


@pytest.mark.parametrize('name', list(TABLE_CASES))
def test_tables_against_the_restatement(name):
    counts, T, K, _ = TABLE_CASES[name]
    (scores, classes, flags, iou), ref = _table_ref(name)
    ev = _evaluator(len(counts), list(np.linspace(0.2, 0.95, T)), K, capacity=len(scores) + 7)
    _fill(ev, scores, classes, flags, iou)
    ev.enqueue()
    got = ev.result()
    assert got['n'] == len(scores) and got['lost'] == 0
    _compare_tables(got, ref, len(scores))
    assert np.array_equal(got['entries'][0, :-1], np.asarray(counts)) and int(got['entries'][0, -1]) == len(scores)
    # the sorted order itself: class, score descending, arrival
    cls, sc, words, bits = ev.sorted()
    order, _ = R.sorted_scopes(scores, classes.astype(np.int64), len(counts))
    assert np.array_equal(cls, classes[order]) and np.array_equal(sc, scores[order]) and np.array_equal(words, flags[order])
    assert np.array_equal(bits, iou[order].view(np.uint32))
    # evaluate() is the restatement's formulas on the device's numbers: bitwise
    from ood_object_detection_amd.effdet.evaluation.calibration_evaluator import calibration_metrics
    for t in range(T):
        a, b = R.metrics(got, t), calibration_metrics(got, t)
        assert all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for k in a), (t, a, b)


def test_mass_bin_boundaries_are_exact():
    """no entry ignored: bin k of a scope with m entries holds floor((k + 1) m / K) - floor(k m / K) of them, whatever the ties"""
    counts, K = [1, 7, 64, 4097, 0, 1000], 64
    scores, classes, flags, iou = _entries_case(counts, 1, 77, ties=3, ignore=False)
    ev = _evaluator(len(counts), [0.5], K, capacity=len(scores))
    _fill(ev, scores, classes, flags, iou)
    ev.enqueue()
    n = ev.result()['bins']['n'][0, :, 1]
    for s, m in enumerate(counts + [sum(counts)]):
        assert n[s].tolist() == [((k + 1) * m) // K - (k * m) // K for k in range(K)], s


# ------------------------------------------------------------------------------------------------ end to end, determinism, capture
def _mechanics_case():
    C, M, n_det, thresholds = 4, 40, 50, [0.5, 0.75]
    return O.dense_case(31, 6, C, M, n_det, 0.0, difficult_frac=0.2), C, M, n_det, thresholds


def _run_split(ev, images, parts, n_det, M):
    ev.clear()
    for idx in np.array_split(np.arange(len(images)), parts):
        ev.add_batch(*_pack([images[i] for i in idx], n_det, M))
    ev.enqueue()
    return ev.result()['block'].copy()


def test_evaluate_end_to_end_and_bit_identical_across_runs_and_splits():
    images, C, M, n_det, thresholds = _mechanics_case()
    ev = _evaluator(C, thresholds, 10, score_threshold=0.05, capacity=4096)
    blocks = [_run_split(ev, images, parts, n_det, M) for parts in (1, 3, len(images), 1)]
    for b in blocks[1:]:
        assert np.array_equal(b, blocks[0])
    acc = R.accumulate(images, C, thresholds, 0.05)
    ref = R.tables(acc['scores'], acc['classes'], acc['flags'], acc['iou'], C, len(thresholds), 10)
    got = ev.result()
    n = len(acc['scores'])
    assert got['n'] == n and n > 100 and np.array_equal(got['gt_count'], acc['gt_count']) and np.array_equal(got['correct'], acc['correct'])
    _compare_tables(got, ref, n)
    out = ev.evaluate()
    # end to end: every metric within n 2^-52 relative of the restatement's
    for t, thr in enumerate(thresholds):
        m = R.metrics(ref, t)
        for k, v in m.items():
            g = out['Calibration/%s@%sIOU' % (k, thr)]
            print('%s@%s: device %.17g restatement %.17g, relative difference %.3e (bound %.3e)'
                  % (k, thr, g, v, abs(g - v) / abs(v) if v else abs(g - v), n * 2.0 ** -52))
            assert abs(g - v) <= n * 2.0 ** -52 * abs(v), (k, thr)
        d = out['Reliability@%sIOU' % thr]
        assert np.array_equal(d['count'], ref['bins']['n'][t, C, 0]) and int(d['count'].sum()) == int(ref['bins']['n'][t, C, 0].sum())


def test_add_batch_and_enqueue_in_a_captured_graph():
    images, C, M, n_det, thresholds = _mechanics_case()
    ev = _evaluator(C, thresholds, 10, capacity=4096)
    a1, a2 = _pack(images[:3], n_det, M), _pack(images[3:], n_det, M)
    ev.add_batch(*a1)
    ev.add_batch(*a2)
    ev.enqueue()
    eager = ev.result()['block']
    ev.clear()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ev.add_batch(*a1)
        ev.add_batch(*a2)
        ev.enqueue()
    ev.clear()
    ev._result.zero_()
    graph.replay()
    assert np.array_equal(ev.result()['block'], eager)


def test_overflow_is_counted_and_result_raises():
    images, C, M, n_det, thresholds = _mechanics_case()
    total = len(R.accumulate(images, C, thresholds)['scores'])
    ev = _evaluator(C, thresholds, 10, capacity=total - 9)
    ev.add_batch(*_pack(images, n_det, M))
    ev.enqueue()
    assert int(ev._state[0]) == total - 9 and int(ev._state[1]) == 9
    with pytest.raises(RuntimeError):
        ev.result()
    ev.clear()
    ev.add_batch(*_pack(images[:2], n_det, M))
    ev.enqueue()
    assert ev.result()['lost'] == 0


def test_single_image_api():
    images, C, M, n_det, thresholds = _mechanics_case()
    ev = _evaluator(C, thresholds, 10, capacity=4096)
    want = _run_split(ev, images, 1, n_det, M)
    ev.clear()
    for i, im in enumerate(images):
        ev.add_single_ground_truth_image_info(i, dict(bbox=im['gt_boxes'], cls=np.asarray(im['gt_classes']) + 1, difficult=im['gt_difficult']))
    for i, im in enumerate(images):
        ev.add_single_detected_image_info(i, dict(bbox=im['det_boxes'], scores=im['det_scores'], cls=np.asarray(im['det_classes']) + 1))
    ev.enqueue()
    assert np.array_equal(ev.result()['block'], want)


# ------------------------------------------------------------------------------------------------ fit
_FIT = {}


def _fit_case(case):
    if case not in _FIT:
        n, a0, b0 = R.FIT_CASES[case]
        _FIT[case] = R.bernoulli_case(100 + case, n, a0, b0)
    return _FIT[case]


@pytest.mark.parametrize('case', range(len(R.FIT_CASES)))
def test_fit_against_the_restatement(case):
    from ood_object_detection_amd.calibration import DetectionCalibrator
    s, f, u = _fit_case(case)
    n = len(s)
    # the same labels at both thresholds; every seventh entry is ignored at threshold 1 only: it takes part at 0
    f = np.where(np.arange(n) % 7 == 0, f | np.uint32(1 << 17), f | (f << np.uint32(1))).astype(np.uint32)
    ev = _evaluator(1, [0.5, 0.75], 2, capacity=n + 11)
    _fill(ev, s, np.zeros(n, np.int32), f, u)
    for target in ('tp', 'iou'):
        x, y = R.fit_data(s, f, u, 0, target)
        for method in ('platt', 'temperature'):
            ref = R.newton_fit(x, y, method, summation='pairwise')
            got = DetectionCalibrator(method, target, DEV).fit(ev).finish()
            print('fit %d %s %s: device - restatement a %.3e b %.3e, %d evaluations' % (case, target, method, got['a'] - ref['a'],
                                                                                       got['b'] - ref['b'], got['iterations']))
            assert got['converged'] and got['iterations'] == ref['iterations'] and got['halvings'] == ref['halvings'] == 0
            assert got['entries'] == n
            assert abs(got['a'] - ref['a']) <= FIT_TOL * max(1.0, abs(ref['a'])) and abs(got['b'] - ref['b']) <= FIT_TOL * max(1.0, abs(ref['b']))
            assert got['nll_after'] <= got['nll_before'] and abs(got['nll_after'] - ref['nll_after']) <= n * 2.0 ** -50 * ref['nll_after']
    # threshold 1 leaves the ignored seventh out
    got = DetectionCalibrator('platt', 'tp', DEV).fit(ev, threshold_index=1).finish()
    assert got['entries'] == n - len(range(0, n, 7))


def test_fit_captured_equals_eager_and_constant_targets_do_not_converge():
    from ood_object_detection_amd.calibration import DetectionCalibrator
    s, f, u = _fit_case(1)
    ev = _evaluator(1, [0.5], 2, capacity=len(s))
    _fill(ev, s, np.zeros(len(s), np.int32), f, u)
    cal = DetectionCalibrator('platt', 'iou', DEV)
    eager = cal.fit(ev).state.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cal.fit(ev)
    cal.state.zero_()
    graph.replay()
    assert torch.equal(cal.state.view(torch.int64), eager.view(torch.int64)) and cal.finish()['converged']
    # separable data: every target 1.  "Not converged", never NaN; finish() raises
    _fill(ev, s, np.zeros(len(s), np.int32), np.ones_like(f), u)
    cal = DetectionCalibrator('platt', 'tp', DEV).fit(ev)
    st = cal.state.cpu().numpy()
    assert st[11] == 0 and np.isfinite(st).all() and 1 <= st[9] <= 32
    with pytest.raises(RuntimeError):
        cal.finish()
    ev.clear()                                                                # no entries at all
    cal = DetectionCalibrator('platt', 'tp', DEV).fit(ev, max_iter=3)
    assert cal.state.cpu().numpy()[:2].tolist() == [1.0, 0.0]
    with pytest.raises(RuntimeError):
        cal.finish()


# ------------------------------------------------------------------------------------------------ apply
@pytest.mark.parametrize('a,b', [(1.5, -0.5), (0.05, 2.0), (8.0, 0.0)])
def test_apply(a, b):
    from ood_object_detection_amd.calibration import DetectionCalibrator
    rs = np.random.RandomState(4)
    B, max_det = 3, 300
    det = rs.uniform(0, 1, (B, max_det, 6)).astype(np.float32)
    det[:, :, 4] = -np.sort(-det[:, :, 4], axis=1)
    det[0, 0, 4], det[0, 299, 4] = 1.0, 0.0
    cnt = np.array([300, 17, 0], np.int32)
    cal = DetectionCalibrator(device=DEV).load_state_dict(dict(a=a, b=b, method='platt', target='tp'))
    d = torch.from_numpy(det).to(DEV)
    with pytest.raises(RuntimeError):
        DetectionCalibrator(device=DEV).apply(d, torch.from_numpy(cnt).to(DEV))      # neither fitted nor loaded
    out = cal.apply(d, torch.from_numpy(cnt).to(DEV))
    assert torch.equal(d.cpu(), torch.from_numpy(det))                        # the input is left alone
    got, ref = out.cpu().numpy(), R.apply_det(det, cnt, a, b)
    mask = np.ones(det.shape, bool)
    for i in range(B):
        mask[i, :cnt[i], 4] = False
    assert np.array_equal(got[mask].view(np.uint32), det[mask].view(np.uint32))
    g, r = got[~mask], ref[~mask]
    assert (np.abs(g.view(np.int32).astype(np.int64) - r.view(np.int32).astype(np.int64)) <= 1).all()
    for i in range(B):
        assert (np.diff(got[i, :cnt[i], 4]) <= 0).all()
    same = cal.apply(d, torch.from_numpy(cnt).to(DEV), out=d)                 # in place
    assert same is d and torch.equal(d, out)


# ------------------------------------------------------------------------------------------------ the chain
def _overconfident_case(seed, n_img, M, n_det):
    """one class; a detection of score p is a true positive (a copy of a ground-truth box no other detection uses) with probability
    sigmoid(0.5 logit(p) - 1.5), else a box far from every ground-truth box: the scores say far more than they deliver"""
    rs = np.random.RandomState(seed)
    images = []
    for _ in range(n_img):
        gt = np.array([[30.0 * (k // 10), 30.0 * (k % 10), 30.0 * (k // 10) + 10, 30.0 * (k % 10) + 10] for k in range(M)], np.float32)
        sc = -np.sort(-rs.uniform(0.05, 0.99, n_det).astype(np.float32))
        q = R.sigmoid(0.5 * R.logit(sc) - 1.5)
        boxes, free = [], list(rs.permutation(M))
        for k in range(n_det):
            if rs.uniform() < q[k] and free:
                boxes.append(gt[free.pop()])
            else:
                boxes.append(np.array([1000, 1000, 1010, 1010], np.float32) + rs.uniform(0, 100))
        images.append(dict(gt_boxes=gt, gt_classes=np.zeros(M, np.int64), det_boxes=np.stack(boxes), det_scores=sc,
                           det_classes=np.zeros(n_det, np.int64)))
    return images


def test_fit_apply_evaluate_chain_in_one_capture_lowers_the_nll():
    from ood_object_detection_amd.calibration import DetectionCalibrator
    images = _overconfident_case(9, 8, 60, 60)
    det, cnt, gtb, gtc, gtd = _pack(images, 60, 60)
    ev1, ev2 = _evaluator(1, [0.5], 10, capacity=1024), _evaluator(1, [0.5], 10, capacity=1024)
    cal = DetectionCalibrator('platt', 'tp', DEV)

    def chain():
        ev1.add_batch(det, cnt, gtb, gtc, gtd)
        ev1.enqueue()
        cal.fit(ev1)
        ev2.add_batch(cal.apply(det, cnt), cnt, gtb, gtc, gtd)
        ev2.enqueue()

    chain()
    eager = (ev1.result()['block'].copy(), ev2.result()['block'].copy(), cal.state.clone())
    ev1.clear(), ev2.clear()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain()
    ev1.clear(), ev2.clear()
    ev1._result.zero_(), ev2._result.zero_(), cal.state.zero_()
    graph.replay()
    r1, r2 = ev1.result(), ev2.result()
    assert np.array_equal(r1['block'], eager[0]) and np.array_equal(r2['block'], eager[1])
    assert torch.equal(cal.state.view(torch.int64), eager[2].view(torch.int64))
    fit = cal.finish()
    assert fit['converged'] and fit['a'] > 0 and fit['nll_after'] < fit['nll_before']
    assert r1['n'] == r2['n'] == 8 * 60 and np.array_equal(r1['bins']['tp'][0, 1].sum(1), r2['bins']['tp'][0, 1].sum(1))
    assert float(r2['nll'][0, 1]) < float(r1['nll'][0, 1])                     # the exact property of the fit
    from ood_object_detection_amd.effdet.evaluation.calibration_evaluator import calibration_metrics
    assert calibration_metrics(r2, 0)['D-ECE'] < calibration_metrics(r1, 0)['D-ECE']


def test_det_bench_predict_with_a_calibrator():
    from _models import seeded_model
    from _seeded import seeded_array
    from ood_object_detection_amd.calibration import DetectionCalibrator
    from ood_object_detection_amd.effdet.bench import DetBenchPredict
    model, _, _, _ = seeded_model('tf_efficientdet_d0', 128, 3, seed=21, cls_bias=-2.0)
    model = model.to(DEV)
    x = torch.from_numpy(seeded_array(22, 'input', (2, 3, 128, 128))).to(DEV)
    plain = DetBenchPredict(model, streams=1).to(DEV)
    with torch.no_grad():
        det0 = plain._forward(x, None).clone()                                # the path without the hook
    cnt0 = plain.last_count.clone()
    assert int(cnt0.sum()) > 0
    assert plain.calibrator is None and torch.equal(plain(x), det0) and torch.equal(plain.last_count, cnt0)
    cal = DetectionCalibrator(device=DEV).load_state_dict(dict(a=0.7, b=-0.4, method='platt', target='tp'))
    bench = DetBenchPredict(model, streams=1, calibrator=cal).to(DEV)
    det1 = bench(x)
    assert torch.equal(det1, cal.apply(det0, cnt0)) and torch.equal(bench.last_count, cnt0) and not torch.equal(det1, det0)
    assert set(bench.last_ood) == set(plain.last_ood)
