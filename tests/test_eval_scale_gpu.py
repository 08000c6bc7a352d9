"""csrc/eval_scale.hip on the device (-m gpu): matching at several IoU thresholds with `difficult` ground truth, the append, the
sorted AP and the evaluators on top, against tests/_eval_scale_ref.py (pinned to the reference's evaluator by
tests/golden/evaluation_scale.npz), against `effdet_eval_match` / `effdet_eval_ap`, and against themselves (bit-identical runs).

Flag words and counters are compared EXACTLY.  AP tolerance, derived: both sides add k products of a float64 recall step and a
precision <= 1, each with a few 2^-53 roundings, k = the class's true positives, so |dAP| <= 4 (k + 1) 2^-52; 1e-12 as in
test_evaluation_gpu.py wherever k <= 1000."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _eval_scale_ref as R
from _seeded import eval_case, eval_case_dense

DEV = 'cuda:0'
INVALID = -2 ** 31


def _cats(C):
    return [{'id': i + 1, 'name': 'c%d' % i} for i in range(C)]


def _dataset(C, thresholds=(0.5,), **kw):
    from ood_object_detection_amd.effdet.evaluation import DatasetDetectionEvaluator
    return DatasetDetectionEvaluator(_cats(C), iou_thresholds=thresholds, device=DEV, **kw)


def _golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'evaluation_scale.npz'))


def _pack(images, max_det, M):
    """0-based images (tests/_eval_scale_ref.py layout) -> det [B,max_det,6] x1,y1,x2,y2,score,class (1-based), count [B],
    gt_boxes [B,M,4], gt_cls [B,M] (1-based, -1 padding), gt_difficult [B,M] uint8"""
    B = len(images)
    det = torch.zeros(B, max_det, 6)
    cnt = torch.zeros(B, dtype=torch.int32)
    gtb, gtc, gtd = torch.zeros(B, M, 4), torch.full((B, M), -1, dtype=torch.int64), torch.zeros(B, M, dtype=torch.uint8)
    for i, im in enumerate(images):
        n = len(im['det_scores'])
        b = torch.from_numpy(np.asarray(im['det_boxes'], np.float32).reshape(-1, 4))
        det[i, :n] = torch.stack([b[:, 1], b[:, 0], b[:, 3], b[:, 2], torch.from_numpy(np.asarray(im['det_scores'], np.float32)),
                                  torch.from_numpy(np.asarray(im['det_classes']) + 1).float()], 1)
        cnt[i] = n
        m = len(im['gt_classes'])
        gtb[i, :m] = torch.from_numpy(np.asarray(im['gt_boxes'], np.float32).reshape(-1, 4))
        gtc[i, :m] = torch.from_numpy(np.asarray(im['gt_classes'], np.int64) + 1)
        if 'gt_difficult' in im:
            gtd[i, :m] = torch.from_numpy(np.asarray(im['gt_difficult']).astype(np.uint8))
    return [t.to(DEV) for t in (det, cnt, gtb, gtc, gtd)]


def _ap_bound(flags, classes, C, t=0):
    """[C] 4 (k + 1) 2^-52 with k the class's true positives at threshold t; 1e-12 instead where k <= 1000"""
    flags, classes = np.asarray(flags).astype(np.int64) & 0xFFFFFFFF, np.asarray(classes)
    k = np.array([int((((flags >> t) & 1) == 1)[(classes == c) & ((flags >> 31) == 0)].sum()) for c in range(C)])
    bound = 4.0 * (k + 1) * 2.0 ** -52
    assert bound.max() < 2e-11
    return np.where(k <= 1000, np.minimum(bound, 1e-12), bound)


def _assert_ap(ap, ref, bound):
    assert np.array_equal(np.isnan(ap), np.isnan(ref)), (ap, ref)
    err = np.abs(np.nan_to_num(ap) - np.nan_to_num(ref))
    print('AP error', err.max(), 'bound', bound.min())
    assert (err <= bound).all(), (err, bound)


# ------------------------------------------------------------------------------------------------ matching
@pytest.mark.parametrize('M', [1, 64, 256, 257, 300])
def test_match_multi_single_threshold_equals_eval_match(M):
    from ood_object_detection_amd.effdet.evaluation import ObjectDetectionEvaluator
    C, n_det = 5, 120
    images = [R.zero_based(im) for im in eval_case_dense(70 + M, 3, C, M, n_det, cls=2)]
    det, cnt, gtb, gtc, _ = _pack(images, n_det + 2, M)
    old = ObjectDetectionEvaluator(_cats(C), evaluate_corlocs=True, device=DEV, ap_method='rank')
    tp = old.add_batch(det, cnt, gtb, gtc).cpu().numpy()
    new = _dataset(C)
    flags = new.add_batch(det, cnt, gtb, gtc).cpu().numpy()
    assert (tp == 1).any() and (tp == 0).any() and (tp == -1).any()
    assert np.array_equal(flags == 1, tp == 1) and np.array_equal(flags == 0, tp == 0) and np.array_equal(flags == INVALID, tp == -1)
    for a, b in ((new._gt_count, old._gt_count), (new._gt_imgs, old._gt_imgs), (new._correct, old._correct)):
        assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    assert int(new._state[0]) == int((tp >= 0).sum()) and new._state[1:].cpu().tolist() == [0, 0, 0]


def _tie_image(ja, jb, M=300):
    """test_evaluation_gpu.py::_tie_image, 0-based: ground truth A = [0,0,10,10] at row ja and B = [0,10,10,20] at row jb, one
    class; detections D = [0,0,10,20] (IoU 0.5 with A and with B), D again, then A itself and B itself"""
    gt = np.zeros((M, 4), np.float32)
    for k in range(M):
        gt[k] = (100 + 30.0 * (k // 20), 30.0 * (k % 20), 110 + 30.0 * (k // 20), 30.0 * (k % 20) + 10)
    gt[ja], gt[jb] = (0, 0, 10, 10), (0, 10, 10, 20)
    det = np.array([[0, 0, 10, 20], [0, 0, 10, 20], [0, 0, 10, 10], [0, 10, 10, 20]], np.float32)
    return dict(gt_boxes=gt, gt_classes=np.zeros(M, np.int64), det_boxes=det,
                det_scores=np.array([0.9, 0.8, 0.7, 0.6], np.float32), det_classes=np.zeros(4, np.int64))


def _multi_cases():
    rs = np.random.RandomState(11)
    C = 5
    for M in (257, 300):
        images = [R.zero_based(im) for im in eval_case_dense(270 + M, 3, C, M, 120, cls=2)]
        for im in images:
            im['gt_difficult'] = rs.uniform(size=M) < 0.3
        yield 'dense %d' % M, images, C, 122, M + 1
    for ja, jb, dif in ((5, 5 + 256, jb_dif) for jb_dif in (0, 1, 2)):
        im = _tie_image(ja, jb)
        d = np.zeros(300, bool)
        if dif:
            d[ja if dif == 1 else jb] = True                                  # the tie goes to A whether A is difficult or not
        im['gt_difficult'] = d
        yield 'tie %d' % dif, [im, im], 2, 4, 300
    # a duplicate ground-truth pair of which one is difficult (either one), detections at IoU exactly 0.5 and exactly 0.75
    gt = np.array([[0, 0, 10, 10], [0, 0, 10, 10], [50, 50, 60, 60], [100, 0, 110, 40], [200, 0, 210, 40]], np.float32)
    det = np.array([[0, 0, 10, 10], [0, 0, 10, 10], [50, 50, 60, 70], [100, 0, 110, 30], [200, 0, 210, 30], [0, 0, 10, 10]], np.float32)
    assert R.iou_matrix(det[2:3], gt[2:3])[0, 0] == np.float32(0.5) and R.iou_matrix(det[3:4], gt[3:4])[0, 0] == np.float32(0.75)
    for k, dif in enumerate(([1, 0, 0, 0, 0], [0, 1, 0, 0, 1], [0, 0, 1, 1, 0])):
        im = dict(gt_boxes=gt, gt_classes=np.zeros(5, np.int64), det_boxes=det, det_classes=np.zeros(6, np.int64),
                  det_scores=np.array([0.9, 0.8, 0.7, 0.6, 0.5, 0.4], np.float32), gt_difficult=np.array(dif, bool))
        yield 'exact %d' % k, [im], 1, 7, 5


def test_match_multi_thresholds_and_difficult_flags():
    thresholds = (0.5, 0.55, 0.75, 0.9)
    seen = []
    for name, images, C, max_det, M in _multi_cases():
        ev = _dataset(C, thresholds)
        det, cnt, gtb, gtc, gtd = _pack(images, max_det, M)
        flags = ev.add_batch(det, cnt, gtb, gtc, gtd).cpu().numpy()
        r = R.evaluate(images, C, thresholds)
        k = 0
        for i, im in enumerate(images):
            n = len(im['det_scores'])
            ref = r['flags'][k:k + n].astype(np.int64)
            got = flags[i, :n].astype(np.int64) & 0xFFFFFFFF
            assert np.array_equal(got, ref), '%s image %d: flags differ at %s' % (name, i, np.nonzero(got != ref)[0][:8].tolist())
            assert (flags[i, n:] == INVALID).all()
            seen.append(ref)
            k += n
        assert np.array_equal(ev._gt_count.cpu().numpy(), r['gt_count']), name
        assert np.array_equal(ev._gt_imgs.cpu().numpy(), r['gt_imgs']), name
        assert np.array_equal(ev._correct.cpu().numpy().reshape(len(thresholds), C), r['correct']), name
    seen = np.concatenate(seen)
    valid = (seen >> 31) == 0
    assert (valid & (seen & 1 == 1) & (seen & 4 == 0) & ((seen >> 18) & 1 == 0)).any()          # TP at 0.5, FP at 0.75
    assert (valid & ((seen >> 16) & 1 == 1) & ((seen >> 19) & 1 == 0) & (seen & 8 == 0)).any()   # ignored at 0.5, FP at 0.9
    assert (valid & (seen & 0xF == 0xF)).any() and (valid & ((seen >> 16) & 0xF == 0xF)).any()


# ------------------------------------------------------------------------------------------------ sorted AP
def _load(ev, scores, classes, flags, gt_count):
    """put accumulated entries into the evaluator's device buffers directly (what add_batch calls would have left there)"""
    n = len(scores)
    ev.clear()
    ev._bufs[0][:n] = torch.from_numpy(np.asarray(scores, np.float32)).to(DEV)
    ev._bufs[1][:n] = torch.from_numpy(np.asarray(classes, np.int32)).to(DEV)
    ev._bufs[2][:n] = torch.from_numpy(np.asarray(flags, np.int64).astype(np.uint32).view(np.int32)).to(DEV)
    ev._state[0] = n
    ev._gt_count.copy_(torch.from_numpy(np.asarray(gt_count, np.int32)))
    ev._gt_imgs.copy_(torch.from_numpy((np.asarray(gt_count) > 0).astype(np.int32)))


def _rank_ap(scores, classes, flags, gt_count, C):
    """the parent's effdet_eval_ap (ap_method='rank') on the same entries, single threshold"""
    import _hip
    from ood_object_detection_amd import _lib
    lib = _lib.load()
    flags = np.asarray(flags, np.int64)
    tp = np.where((flags >> 31) & 1 == 1, -1, np.where((flags >> 16) & 1 == 1, -1, flags & 1))          # ignored: takes no part
    n = len(scores)
    s = torch.from_numpy(np.asarray(scores, np.float32)).to(DEV)
    c = torch.from_numpy(np.asarray(classes, np.int32)).to(DEV)
    t = torch.from_numpy(tp.astype(np.int32)).to(DEV)
    g = torch.from_numpy(np.asarray(gt_count, np.int32)).to(DEV)
    ap = torch.full((C,), 123.0, dtype=torch.float64, device=DEV)
    nb = lib.effdet_eval_ap_workspace_bytes(n)
    ws = torch.empty((nb + 7) // 8, dtype=torch.float64, device=DEV)
    assert lib.effdet_eval_ap(_hip.stream(DEV), s.data_ptr(), c.data_ptr(), t.data_ptr(), n, C, g.data_ptr(), ap.data_ptr(),
                              ws.data_ptr(), nb) == 0
    return ap.cpu().numpy()


def _tile():
    from ood_object_detection_amd import _lib
    return _lib.load().effdet_eval_scale_sort_tile()


def _entries(n, C, seed, levels=4096):
    rs = np.random.RandomState(seed)
    classes = rs.randint(-1, C, n)
    scores = ((rs.randint(0, levels, n) - levels // 4) / np.float32(levels)).astype(np.float32)
    u = rs.uniform(size=n)
    flags = np.where(u < 0.3, 1, np.where(u < 0.4, 1 << 16, np.where(u < 0.45, 1 << 31, 0))).astype(np.int64)
    gt_count = np.array([int(((flags == 1) & (classes == c)).sum()) + rs.randint(1, 9) for c in range(C)])
    return scores, classes, flags, gt_count


SIZES = ['1', '255', '257', 'tile-1', 'tile', 'tile+1', '3*tile+17', '65536']
# beyond the sizes: 255 classes = five sort passes with the invalid class 255 in the top digit; 256 and 300 = the sixth pass
MANY_CLASSES = [255, 256, 300]


@pytest.mark.parametrize('which,C', [(w, 5) for w in SIZES] + [('tile+1', C) for C in MANY_CLASSES],
                         ids=SIZES + ['tile+1-%d-classes' % C for C in MANY_CLASSES])
def test_sorted_ap_sizes(which, C):
    tile = _tile()
    n = eval(which, {'tile': tile})
    scores, classes, flags, gt_count = _entries(n, C, 1000 + n % 997)
    ev = _dataset(C, capacity=max(n, 2 * tile + 5))
    _load(ev, scores, classes, flags, gt_count)
    ev.enqueue()
    r = ev.result()
    assert r['n'] == n and r['lost'] == 0 and np.array_equal(r['gt_count'], gt_count)
    bound = _ap_bound(flags, classes, C)
    ref = R.ap_from_entries(scores, classes, flags, gt_count, C, 1)[0]
    _assert_ap(r['ap'][0], ref, bound)
    _assert_ap(r['ap'][0], _rank_ap(scores, classes, flags, gt_count, C), bound)
    cls, sc, fl = ev.sorted()
    rc, rs_, rf = R.sorted_entries(scores, classes, flags, C)
    assert np.array_equal(cls, rc) and np.array_equal(sc.view(np.uint32), rs_.view(np.uint32)) and np.array_equal(fl, rf)


def test_sorted_ap_equal_scores_keep_their_arrival_order():
    """8 distinct scores (-0.0 and +0.0 tie), TP flags alternate, so a wrong order inside a tie changes AP; 3 tiles + 17 entries, so
    equal keys straddle waves and tiles.  The unused bits 1..15 of the flag word carry the arrival index."""
    tile = _tile()
    n, C = 3 * tile + 17, 5
    rs = np.random.RandomState(8)
    values = np.array([-1.5, -0.0, 0.0, 0.125, 0.25, 0.5, 0.75, 1.0, 3.0], np.float32)
    scores = values[rs.randint(0, len(values), n)]
    assert len(np.unique(scores)) == 8 and np.signbit(scores[scores == 0]).any() and (~np.signbit(scores[scores == 0])).any()
    classes = rs.randint(0, C, n)
    flags = (np.arange(n) % 2) | ((np.arange(n) & 0x7FFF) << 1)
    gt_count = np.array([int(((flags & 1 == 1) & (classes == c)).sum()) + 3 for c in range(C)])
    ev = _dataset(C, capacity=n + 100)
    _load(ev, scores, classes, flags, gt_count)
    ev.enqueue()
    cls, sc, fl = ev.sorted()
    rc, rsc, rf = R.sorted_entries(scores, classes, flags, C)
    assert np.array_equal(cls, rc) and np.array_equal(fl, rf) and np.array_equal(sc.view(np.uint32), rsc.view(np.uint32))
    assert not np.signbit(sc).any() or (sc[np.signbit(sc)] < 0).all()                       # -0.0 came out as +0.0
    ap = ev.result()['ap'][0]
    _assert_ap(ap, R.ap_from_entries(scores, classes, flags, gt_count, C, 1)[0], _ap_bound(flags, classes, C))
    # the check has teeth: ties resolved the other way round give another AP
    rev = R.ap_from_entries(scores[::-1], classes[::-1], flags[::-1], gt_count, C, 1)[0]
    assert np.abs(rev - ap).max() > 1e-6


def test_sorted_ap_special_classes_and_entries_that_must_not_count():
    """class 0: ground truth, no detection -> 0; class 1: detections, no ground truth -> NaN; class 2: every detection ignored ->
    0; classes 3 and 4 ordinary.  NaN scores, dropped entries and classes outside 0..C-1 sprinkled in change nothing."""
    C, n = 5, 3000
    rs = np.random.RandomState(21)
    classes = rs.choice([1, 2, 3, 4], n)
    scores = rs.permutation(n).astype(np.float32) / n
    flags = np.where(rs.uniform(size=n) < 0.4, 1, 0).astype(np.int64)
    flags[classes == 2] = 1 << 16
    gt_count = np.array([4, 0, 6, int((flags[classes == 3] & 1).sum()) + 2, int((flags[classes == 4] & 1).sum())])
    ev = _dataset(C, thresholds=(0.5,), capacity=8192)
    _load(ev, scores, classes, flags, gt_count)
    ev.enqueue()
    clean = ev.result()
    ap = clean['ap'][0]
    assert ap[0] == 0.0 and np.isnan(ap[1]) and ap[2] == 0.0 and 0 < ap[3] < 1 and 0 < ap[4] <= 1
    _assert_ap(ap, R.ap_from_entries(scores, classes, flags, gt_count, C, 1)[0], _ap_bound(flags, classes, C))
    # the same with 600 entries that take no part, at random places
    m = n + 600
    pos = np.sort(rs.permutation(m)[:n])
    s2, c2, f2 = np.full(m, 0.99, np.float32), rs.randint(0, C, m), np.ones(m, np.int64)
    kind = rs.randint(0, 4, m)
    s2[kind == 0] = np.nan
    f2[kind == 1] = (1 << 31) | 1
    c2[kind == 2] = C
    c2[kind == 3] = -1
    s2[(kind == 1) & (np.arange(m) % 2 == 0)] = np.nan
    s2[pos], c2[pos], f2[pos] = scores, classes, flags
    _load(ev, s2, c2, f2, gt_count)
    ev.enqueue()
    dirty = ev.result()
    assert np.array_equal(dirty['ap'].view(np.int64), clean['ap'].view(np.int64)) and dirty['n'] == m
    cls, sc, fl = ev.sorted()
    assert len(cls) == n and not np.isnan(sc).any()


# ------------------------------------------------------------------------------------------------ threshold sweep
def test_one_evaluator_with_ten_thresholds_equals_ten_evaluators():
    g = _golden()
    images, C = R.fixture_case(g, 'a')
    assert sum(int(im['gt_difficult'].sum()) for im in images) == 13
    thresholds = [round(0.5 + 0.05 * i, 2) for i in range(10)]
    packed = _pack(images, 40, 5)
    ev = _dataset(C, thresholds, evaluate_corlocs=True, capacity=4096)
    ev.add_batch(*packed)
    ev.enqueue()
    sweep = ev.result()
    for t, thr in enumerate(thresholds):
        one = _dataset(C, (thr,), evaluate_corlocs=True, capacity=4096)
        one.add_batch(*packed)
        one.enqueue()
        r = one.result()
        assert np.array_equal(r['ap'][0].view(np.int64), sweep['ap'][t].view(np.int64)), thr
        assert np.array_equal(r['correct'][0], sweep['correct'][t]) and np.array_equal(r['gt_count'], sweep['gt_count'])
    m = ev.evaluate()
    for k, thr in enumerate(g['thresholds']):
        t = thresholds.index(float(thr))
        assert np.allclose(sweep['ap'][t], g['a_ap'][k], rtol=0, atol=1e-12, equal_nan=True)
        assert abs(m['Precision/mAP@{}IOU'.format(float(thr))] - g['a_map'][k]) <= 1e-12
        assert abs(m['Precision/meanCorLoc@{}IOU'.format(float(thr))] - g['a_corloc'][k]) <= 1e-12
        for c in range(C):
            assert np.allclose(m['CorLoc@{}IOU/c{}'.format(float(thr), c)], g['a_cl'][k][c], rtol=0, atol=1e-12, equal_nan=True)
    maps = [m['Precision/mAP@{}IOU'.format(thr)] for thr in thresholds]
    assert m['Precision/mAP@[0.5:0.95]IOU'] == float(np.nanmean(maps))
    assert 'AP@0.6IOU/c0' in m and 'AP@0.95IOU/c5' in m


# ------------------------------------------------------------------------------------------------ scale
def _scale_images(n_img, n_det, M, C, seed):
    """0-based images: M ground-truth 10 x 10 boxes on a grid with random classes; n_det detections with distinct descending
    scores: about 30 % exact copies of DISTINCT ground-truth boxes with their class (true positives), the others far away"""
    rs = np.random.RandomState(seed)
    k = np.arange(M)
    gt = np.stack([30.0 * (k // 20), 30.0 * (k % 20), 30.0 * (k // 20) + 10, 30.0 * (k % 20) + 10], 1).astype(np.float32)
    images = []
    for _ in range(n_img):
        gc = rs.randint(0, C, M)
        hit = rs.uniform(size=n_det) < 0.3
        hit[np.nonzero(hit)[0][M:]] = False
        which = rs.permutation(M)[:hit.sum()]
        box = np.stack([rs.uniform(1000, 2000, n_det), rs.uniform(0, 500, n_det)], 1).astype(np.float32)
        box = np.concatenate([box, box + np.float32(12)], 1)
        dc = rs.randint(0, C, n_det)
        box[hit], dc[hit] = gt[which], gc[which]
        sc = np.sort(rs.permutation(1 << 20)[:n_det].astype(np.float32) / np.float32(1 << 20))[::-1].copy()
        images.append(dict(gt_boxes=gt, gt_classes=gc, det_boxes=box, det_scores=sc, det_classes=dc))
    return images


@pytest.mark.parametrize('total', [65537, 200000])
def test_object_detection_evaluator_beyond_65536_detections(total):
    """the parent raises RuntimeError here ('effdet_eval_ap handles 65536')"""
    from ood_object_detection_amd.effdet.evaluation import ObjectDetectionEvaluator
    C, per, M = 20, 1000, 320
    full, rest = divmod(total, per)
    images = _scale_images(full, per, M, C, total) + (_scale_images(1, rest, M, C, total + 1) if rest else [])
    ev = ObjectDetectionEvaluator(_cats(C), evaluate_corlocs=True, device=DEV)
    ev.add_batch(*_pack(images[:full], per, M)[:4])
    if rest:
        ev.add_batch(*_pack(images[full:], rest, M)[:4])
    assert sum(t.numel() for t in ev._scores) == total
    m = ev.evaluate()
    r = R.evaluate(images, C, [0.5])
    tp_share = float((r['flags'] & 1).mean())
    assert 0.25 < tp_share < 0.35
    ap = np.array([m['AP@0.5IOU/c%d' % c] for c in range(C)])
    _assert_ap(ap, r['ap'][0], _ap_bound(r['flags'], r['classes'], C))
    cl = np.array([m['CorLoc@0.5IOU/c%d' % c] for c in range(C)])
    assert np.allclose(cl, r['corloc'][0], rtol=0, atol=1e-12, equal_nan=True)
    assert abs(m['Precision/mAP@0.5IOU'] - r['mean_ap'][0]) <= _ap_bound(r['flags'], r['classes'], C).max()


def test_pascal_evaluator_with_difficult_ground_truth_matches_the_reference():
    """the parent raises NotImplementedError at the 'difficult' key"""
    from ood_object_detection_amd.effdet.evaluation import PascalDetectionEvaluator
    g = _golden()
    for tag in ('a', 'b'):
        seed, n_img, C, n_det = [int(v) for v in g[tag + '_meta']]
        images = eval_case(seed, n_img, C, n_det)
        zb, _ = R.fixture_case(g, tag)
        for k, thr in enumerate(g['thresholds']):
            ev = PascalDetectionEvaluator(_cats(C), matching_iou_threshold=float(thr), device=DEV)
            for i, im in enumerate(images):
                ev.add_single_ground_truth_image_info(i, {'bbox': im['gt_boxes'], 'cls': im['gt_classes'], 'difficult': zb[i]['gt_difficult']})
            for i, im in enumerate(images):
                ev.add_single_detected_image_info(i, {'bbox': im['det_boxes'], 'scores': im['det_scores'], 'cls': im['det_classes']})
            m = ev.evaluate()
            ap = np.array([m['AP@{}IOU/c{}'.format(float(thr), c)] for c in range(C)])
            assert np.allclose(ap, g[tag + '_ap'][k], rtol=0, atol=1e-12, equal_nan=True), (tag, thr)
            assert abs(m['PascalBoxes_Precision/mAP@{}IOU'.format(float(thr))] - g[tag + '_map'][k]) <= 1e-12


def test_dataset_evaluator_single_image_api_and_images_without_detections():
    g = _golden()
    images, C = R.fixture_case(g, 'b')
    ev = _dataset(C, (0.5, 0.55, 0.75), evaluate_corlocs=True, capacity=4096)
    for i, im in enumerate(images):
        ev.add_single_ground_truth_image_info(i, {'bbox': im['gt_boxes'], 'cls': im['gt_classes'] + 1, 'difficult': im['gt_difficult']})
    for i, im in enumerate(images[:-1]):                                                    # the last image never gets detections
        ev.add_single_detected_image_info(i, {'bbox': im['det_boxes'], 'scores': im['det_scores'], 'cls': im['det_classes'] + 1})
    with pytest.raises(NotImplementedError):
        ev.add_single_ground_truth_image_info(99, {'bbox': np.zeros((0, 4)), 'cls': np.zeros(0), 'group_of': np.zeros(0)})
    ev.enqueue()
    r = ev.result()
    last = dict(images[-1], det_boxes=np.zeros((0, 4), np.float32), det_scores=np.zeros(0, np.float32), det_classes=np.zeros(0, np.int64))
    ref = R.evaluate(images[:-1] + [last], C, (0.5, 0.55, 0.75))
    assert np.allclose(r['ap'], ref['ap'], rtol=0, atol=1e-12, equal_nan=True)
    assert np.array_equal(r['gt_count'], ref['gt_count']) and np.array_equal(r['gt_imgs'], ref['gt_imgs']) and np.array_equal(r['correct'], ref['correct'])


# ------------------------------------------------------------------------------------------------ mechanics
def _fixture_packed():
    g = _golden()
    images, C = R.fixture_case(g, 'a')
    return images, C, (0.5, 0.55, 0.75)


def _run_split(ev, images, parts):
    ev.clear()
    for idx in np.array_split(np.arange(len(images)), parts):
        ev.add_batch(*_pack([images[i] for i in idx], 40, 5))
    ev.enqueue()
    return ev.result()['block']


def test_result_block_is_bit_identical_across_runs_and_splits():
    images, C, thresholds = _fixture_packed()
    ev = _dataset(C, thresholds, capacity=4096)
    blocks = [_run_split(ev, images, parts) for parts in (1, 3, 7, 1)]
    for b in blocks[1:]:
        assert np.array_equal(b, blocks[0])
    other = _dataset(C, thresholds, capacity=1 << 16)
    assert np.array_equal(_run_split(other, images, 2), blocks[0])
    assert blocks[0][0] == int(((R.evaluate(images, C, thresholds)['flags'] >> 31) == 0).sum())


def test_add_batch_and_enqueue_in_a_captured_graph():
    images, C, thresholds = _fixture_packed()
    ev = _dataset(C, thresholds, capacity=4096)
    first, second = _pack(images[:4], 40, 5), _pack(images[4:], 40, 5)
    ev.add_batch(*first)
    ev.add_batch(*second)
    ev.enqueue()
    eager = ev.result()['block']
    ev.clear()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ev.add_batch(*first)
        ev.add_batch(*second)
        ev.enqueue()
    for _ in range(2):
        ev.clear()
        ev._result.zero_()
        graph.replay()
        assert np.array_equal(ev.result()['block'], eager)


def test_overflow_is_reported_and_clear_allows_reuse():
    C = 3
    rs = np.random.RandomState(4)
    images = []
    for _ in range(12):
        y = rs.uniform(0, 100, 100).astype(np.float32)
        box = np.stack([y, y, y + 10, y + 10], 1)
        images.append(dict(gt_boxes=box[:3], gt_classes=np.array([0, 1, 2]), det_boxes=box, det_classes=rs.randint(0, C, 100),
                           det_scores=np.sort(rs.uniform(size=100).astype(np.float32))[::-1].copy()))
    ev = _dataset(C, capacity=1000)
    ev.add_batch(*_pack(images[:7], 100, 3))
    ev.add_batch(*_pack(images[7:], 100, 3))
    ev.enqueue()
    with pytest.raises(RuntimeError, match=r'\b200\b.*\b1000\b'):
        ev.result()
    ev.clear()
    ev.add_batch(*_pack(images[:10], 100, 3))
    ev.enqueue()
    r = ev.result()
    assert r['n'] == 1000 and r['lost'] == 0
    assert np.allclose(r['ap'], R.evaluate(images[:10], C, (0.5,))['ap'], rtol=0, atol=1e-12, equal_nan=True)


def test_nan_scores_are_counted_and_dropped():
    images, C, thresholds = _fixture_packed()
    ev = _dataset(C, thresholds, capacity=4096)
    det, cnt, gtb, gtc, gtd = _pack(images, 40, 5)
    clean = R.evaluate(images, C, thresholds)
    det[2, 5, 4] = float('nan')
    det[7, 0, 4] = float('nan')
    flags = ev.add_batch(det, cnt, gtb, gtc, gtd).cpu().numpy()
    assert flags[2, 5] == INVALID and flags[7, 0] == INVALID
    ev.enqueue()
    r = ev.result()
    assert r['nan_scores'] == 2
    dirty = [dict(im) for im in images]
    for i, j in ((2, 5), (7, 0)):
        s = dirty[i]['det_scores'].copy()
        s[j] = np.nan
        dirty[i]['det_scores'] = s
    ref = R.evaluate(dirty, C, thresholds)
    assert np.allclose(r['ap'], ref['ap'], rtol=0, atol=1e-12, equal_nan=True) and r['n'] == int(((ref['flags'] >> 31) == 0).sum())
    assert clean['ap'].shape == ref['ap'].shape


class _Spy(object):
    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*a):
            self.calls.append(name)
            return fn(*a)
        return call


def test_auto_runs_the_two_entry_points_of_the_training_loop():
    from ood_object_detection_amd.effdet.evaluation import ObjectDetectionEvaluator
    C = 6
    images = [R.zero_based(im) for im in eval_case(31, 10, C, 40)]
    det, cnt, gtb, gtc, gtd = _pack(images, 40, 5)
    assert not gtd.any()
    runs = {}
    for method, difficult in (('rank', None), ('auto', None), ('auto', gtd), ('sort', None)):
        ev = ObjectDetectionEvaluator(_cats(C), evaluate_corlocs=True, device=DEV, ap_method=method)
        ev.lib = _Spy(ev.lib)
        ev.add_batch(det, cnt, gtb, gtc) if difficult is None else ev.add_batch(det, cnt, gtb, gtc, difficult)
        runs[(method, difficult is not None)] = (ev.evaluate(), [c for c in ev.lib.calls if not c.endswith('_bytes')])
    for key in (('rank', False), ('auto', False), ('auto', True)):                          # all-false flags = no flags
        assert runs[key][1] == ['effdet_eval_match', 'effdet_eval_ap'], key
        assert all(np.array_equal(v, runs[('rank', False)][0][k], equal_nan=True) for k, v in runs[key][0].items())
    assert runs[('sort', False)][1] == ['effdet_eval_match_multi', 'effdet_eval_ap_sorted']
    for k, v in runs[('sort', False)][0].items():
        assert np.allclose(v, runs[('rank', False)][0][k], rtol=0, atol=1e-12, equal_nan=True), k
    with pytest.raises(NotImplementedError):
        ObjectDetectionEvaluator(_cats(C), device=DEV, ap_method='rank').add_batch(det, cnt, gtb, gtc, gtd)
    with pytest.raises(NotImplementedError):
        ObjectDetectionEvaluator(_cats(C), device=DEV, ap_method='rank').add_single_ground_truth_image_info(
            0, {'bbox': np.zeros((1, 4)), 'cls': np.ones(1), 'difficult': np.zeros(1)})


def test_sorted_path_is_faster_than_rank_counting_at_65536():
    """the sanity condition on the sort: at the largest size `effdet_eval_ap` takes (4.3e9 pair comparisons there), a handful of
    passes over 65 536 keys must be the faster way; both timed by device events after one warm-up call"""
    n, C = 65536, 5
    scores, classes, flags, gt_count = _entries(n, C, 77)
    ev = _dataset(C, capacity=n)
    _load(ev, scores, classes, flags, gt_count)

    def timed(fn):
        fn()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1)
    t_sort = timed(ev.enqueue)
    t_rank = timed(lambda: _rank_ap(scores, classes, flags, gt_count, C))
    print('enqueue %.3f ms, effdet_eval_ap with its copies %.3f ms' % (t_sort, t_rank))
    assert t_sort < t_rank


def test_sixteen_thresholds_ignored_everywhere_shares_the_dropped_bit():
    """with 16 thresholds `ignored at the 16th` is bit 31: such a detection is ignored at every threshold (they ascend), which is
    what dropping it does; the append leaves no gap behind it"""
    thresholds = [round(0.2 + 0.05 * i, 2) for i in range(16)]
    cases = {name: images for name, images, _, _, _ in _multi_cases() if name.startswith('exact')}
    images = cases['exact 0'] + cases['exact 2'] + cases['exact 1']
    ev = _dataset(1, thresholds, capacity=64)
    flags = ev.add_batch(*_pack(images, 7, 5)).cpu().numpy().astype(np.int64) & 0xFFFFFFFF
    r = R.evaluate(images, 1, thresholds)
    assert np.array_equal(flags[:, :6].reshape(-1), r['flags'].astype(np.int64))
    assert (r['flags'] == 0xFFFF0000).any() and (r['flags'] == 0xFFFF).any()
    ev.enqueue()
    res = ev.result()
    assert res['n'] == int(((r['flags'] >> 31) == 0).sum()) < 18
    assert np.allclose(res['ap'], r['ap'], rtol=0, atol=1e-12, equal_nan=True)
    cls, sc, fl = ev.sorted()
    rc, rsc, rf = R.sorted_entries(r['scores'], r['classes'], r['flags'], 1)
    assert np.array_equal(fl, rf) and np.array_equal(sc, rsc)
