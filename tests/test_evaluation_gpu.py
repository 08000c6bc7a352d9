"""effdet_eval_match / effdet_eval_ap against oracle/evaluation.py (-m gpu), where tests/_seeded.py::eval_case does not reach:
ground truth that fills every lane, every wave and the second loop trip of the matching kernel, ties in IoU and in score,
IoU exactly at the threshold, duplicate ground truth, dropped classes, thousands of detections.

true-positive flags and the three counter arrays are compared EXACTLY (IoU is correctly rounded float32 on both sides); AP
within 1e-12, as in test_kernels_gpu.py::test_detection_evaluator_golden.  oracle/evaluation.py is pinned to the reference's
evaluator by tests/test_oracle_golden.py::test_evaluation_oracle_matches_reference; its rule for equal scores (the one given
first comes first) is the one evaluation.hip documents."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import evaluation as oe

DEV = 'cuda:0'


def _evaluator(C):
    from ood_object_detection_amd.effdet.evaluation import ObjectDetectionEvaluator
    return ObjectDetectionEvaluator([{'id': i + 1, 'name': 'c%d' % i} for i in range(C)], evaluate_corlocs=True, device=DEV)


def _pack(images, max_det, M, counts=None):
    """images (eval_case layout) -> det [B,max_det,6] x1,y1,x2,y2,score,class; count [B]; gt_boxes [B,M,4]; gt_cls [B,M]"""
    B = len(images)
    det = torch.zeros(B, max_det, 6)
    cnt = torch.zeros(B, dtype=torch.int32)
    gtb, gtc = torch.zeros(B, M, 4), torch.full((B, M), -1, dtype=torch.int64)
    for i, im in enumerate(images):
        n = len(im['det_scores'])
        b = torch.from_numpy(np.asarray(im['det_boxes'], np.float32).reshape(-1, 4))
        det[i, :n] = torch.stack([b[:, 1], b[:, 0], b[:, 3], b[:, 2], torch.from_numpy(np.asarray(im['det_scores'], np.float32)),
                                  torch.from_numpy(np.asarray(im['det_classes'])).float()], 1)
        cnt[i] = n if counts is None else counts[i]
        m = len(im['gt_classes'])
        gtb[i, :m] = torch.from_numpy(np.asarray(im['gt_boxes'], np.float32).reshape(-1, 4))
        gtc[i, :m] = torch.from_numpy(np.asarray(im['gt_classes'], np.int64))
    return det, cnt, gtb, gtc


def _zero_based(im, n=None):
    n = len(im['det_scores']) if n is None else n
    return dict(det_boxes=im['det_boxes'][:n], det_scores=im['det_scores'][:n], det_classes=np.asarray(im['det_classes'][:n]) - 1,
                gt_boxes=im['gt_boxes'], gt_classes=np.asarray(im['gt_classes']) - 1)


def _oracle_tp(im, C, n=None):
    """per-detection flags in the device's layout: 1 / 0, -1 for invalid boxes and classes outside 1..C"""
    z = _zero_based(im, n)
    boxes = np.asarray(z['det_boxes'], np.float32).reshape(-1, 4)
    valid = (boxes[:, 0] < boxes[:, 2]) & (boxes[:, 1] < boxes[:, 3])
    _, tps, correct = oe.per_image(z['det_boxes'], z['det_scores'], z['det_classes'], z['gt_boxes'], z['gt_classes'], C)
    out = np.full(len(z['det_scores']), -1, np.int64)
    for c in range(C):
        idx = np.nonzero(valid & (z['det_classes'] == c))[0]
        idx = idx[np.argsort(-np.asarray(z['det_scores'])[idx], kind='stable')]
        assert len(idx) == len(tps[c])
        out[idx] = tps[c].astype(np.int64)
    return out, correct


def _check_batch(ev, images, C, max_det, M, counts=None, base=None):
    """one add_batch against the oracle: flags and counters exact.  `base`: counters before the call."""
    det, cnt, gtb, gtc = _pack(images, max_det, M, counts)
    base = base or [np.zeros(C, np.int64)] * 3
    tp = ev.add_batch(det.to(DEV), cnt.to(DEV), gtb.to(DEV), gtc.to(DEV)).cpu().numpy()
    gt_count, gt_imgs, correct = [b.copy() for b in base]
    for i, im in enumerate(images):
        n = min(int(cnt[i]), max_det)
        ref, cor = _oracle_tp(im, C, n)
        assert np.array_equal(tp[i, :n], ref), 'image %d: flags differ at %s' % (i, np.nonzero(tp[i, :n] != ref)[0][:8].tolist())
        assert (tp[i, n:] == -1).all()
        gc = np.asarray(im['gt_classes'])
        for c in range(C):
            k = int((gc == c + 1).sum())
            gt_count[c] += k
            gt_imgs[c] += 1 if k else 0
        correct += cor
    assert np.array_equal(ev._gt_count.cpu().numpy(), gt_count)
    assert np.array_equal(ev._gt_imgs.cpu().numpy(), gt_imgs)
    assert np.array_equal(ev._correct.cpu().numpy(), correct)
    return tp, [gt_count, gt_imgs, correct]


def _check_metrics(ev, images, C, ns=None):
    with np.errstate(all='ignore'):
        r = oe.evaluate([_zero_based(im, None if ns is None else ns[i]) for i, im in enumerate(images)], C)
    m = ev.evaluate()
    ap = np.array([m['AP@0.5IOU/c%d' % i] for i in range(C)])
    cl = np.array([m['CorLoc@0.5IOU/c%d' % i] for i in range(C)])
    assert np.allclose(ap, r['per_class_ap'], rtol=0, atol=1e-12, equal_nan=True)
    assert np.allclose(cl, r['per_class_corloc'], rtol=0, atol=1e-12, equal_nan=True)
    assert np.allclose(m['Precision/mAP@0.5IOU'], r['mean_ap'], rtol=0, atol=1e-12, equal_nan=True)
    assert np.allclose(m['Precision/meanCorLoc@0.5IOU'], r['mean_corloc'], rtol=0, atol=1e-12, equal_nan=True)
    return ap


# ------------------------------------------------------------------------------------------------ matching
@pytest.mark.parametrize('M', [1, 64, 256, 257, 300])
def test_eval_match_dense_ground_truth(M):
    """all ground truth of one class: lanes 0..63 of every wave and (M > 256) the second trip of the `j += 256` loop hold
    candidates, duplicates of ground-truth boxes tie in IoU; two add_batch calls accumulate the counters"""
    from _seeded import eval_case_dense
    C, n_det = 5, 120
    ev = _evaluator(C)
    first = eval_case_dense(70 + M, 3, C, M, n_det, cls=2)
    second = eval_case_dense(170 + M, 2, C, M, n_det, cls=4)
    tp, base = _check_batch(ev, first, C, n_det + 2, M)
    assert (tp == 1).any() and (tp == 0).any() and (tp == -1).any()
    _check_batch(ev, second, C, n_det, M + 3, base=base)                      # padded ground truth rows, counters go on
    ap = _check_metrics(ev, first + second, C)
    assert np.isfinite(ap[1]) and np.isfinite(ap[3]) and np.isnan(ap[0])
    # a class with detections and no ground truth: NaN; it is there (eval_case_dense gives some detections class cls % C + 1)
    assert any((np.asarray(im['det_classes']) == 3).any() for im in first) and np.isnan(ap[2])


def _tie_image(ja, jb, M=300):
    """ground truth A = [0,0,10,10] at row ja and B = [0,10,10,20] at row jb (ja < jb), everything else far away, one class.
    detections: D = [0,0,10,20] (IoU 0.5 with A and with B: a tie), D again, then A itself and B itself."""
    gt = np.zeros((M, 4), np.float32)
    for k in range(M):
        gt[k] = (100 + 30.0 * (k // 20), 30.0 * (k % 20), 110 + 30.0 * (k // 20), 30.0 * (k % 20) + 10)
    gt[ja], gt[jb] = (0, 0, 10, 10), (0, 10, 10, 20)
    det = np.array([[0, 0, 10, 20], [0, 0, 10, 20], [0, 0, 10, 10], [0, 10, 10, 20]], np.float32)
    return dict(gt_boxes=gt, gt_classes=np.full(M, 1, np.int64), det_boxes=det,
                det_scores=np.array([0.9, 0.8, 0.7, 0.6], np.float32), det_classes=np.full(4, 1, np.int64))


@pytest.mark.parametrize('ja,jb', [(3, 10), (5, 5 + 64), (5, 5 + 256), (70, 70 + 128), (63, 64), (255, 256), (0, 299)])
def test_eval_match_iou_tie_takes_the_lower_row(ja, jb):
    """two ground-truth boxes with the same IoU to a detection, in one wave, in different waves (j, j + 64), in different
    loop trips (j, j + 256): the detection takes the lower row (A).  Like the reference (per_image_evaluation.py:391-405:
    argmax first, then `is the box taken`), a second identical detection finds A again, taken: false positive - it does NOT
    move on to B.  Then A itself is a false positive (taken) and B itself a true positive (still free); had the tie gone to
    the higher row, those two flags would be swapped."""
    C = 2
    im = _tie_image(ja, jb)
    assert oe.iou_matrix(im['det_boxes'][:1], im['gt_boxes'][[ja, jb]]).tolist() == [[0.5, 0.5]]
    ref, _ = _oracle_tp(im, C)
    assert ref.tolist() == [1, 0, 0, 1]
    ev = _evaluator(C)
    tp, _ = _check_batch(ev, [im, im], C, 4, 300)
    assert tp.tolist() == [[1, 0, 0, 1], [1, 0, 0, 1]]


def _just_below_half():
    """ground truth [0, 0, 12, 12] and a detection [0, d, 12, 12 + d] (IoU (12 - d) / (12 + d), 0.5 at d = 4) whose oracle IoU
    is one float32 step below 0.5: the best of the 40 float32 values above d = 4"""
    gt = np.array([[0, 0, 12, 12]], np.float32)
    d, best = np.float32(4), None
    for _ in range(40):
        d = np.nextafter(d, np.float32(100))
        det = np.array([[0, d, 12, np.float32(12) + d]], np.float32)
        v = oe.iou_matrix(det, gt)[0, 0]
        if v < np.float32(0.5) and (best is None or v > best[0]):
            best = (v, det[0])
    assert best[0] == np.nextafter(np.float32(0.5), np.float32(0))
    return gt[0], best[1]


def test_eval_match_iou_exactly_at_the_threshold():
    """IoU exactly 0.5 is a true positive (`>=`), one float32 step below is a false positive"""
    C = 1
    g0, d0 = _just_below_half()
    gt = np.stack([g0, np.array([50, 50, 60, 60], np.float32)])
    det = np.stack([d0, np.array([50, 50, 60, 70], np.float32)])
    assert oe.iou_matrix(det[1:], gt[1:])[0, 0] == np.float32(0.5)
    im = dict(gt_boxes=gt, gt_classes=np.array([1, 1]), det_boxes=det, det_scores=np.array([0.9, 0.8], np.float32),
              det_classes=np.array([1, 1]))
    ev = _evaluator(C)
    tp, _ = _check_batch(ev, [im], C, 2, 2)
    assert tp.tolist() == [[0, 1]]
    assert ev._correct.cpu().tolist() == [0]                                  # CorLoc looks at the top-scoring detection only
    swapped = dict(im, det_boxes=det[::-1].copy())
    ev = _evaluator(C)
    tp, _ = _check_batch(ev, [swapped], C, 2, 2)
    assert tp.tolist() == [[1, 0]] and ev._correct.cpu().tolist() == [1]


def test_eval_match_dropped_classes_counts_and_limits():
    """classes 0, C + 1 and negative in detections and in ground truth are dropped; det_count above max_det is clamped,
    det_count 0 leaves every flag -1"""
    from _seeded import eval_case_dense
    C, M, n_det = 4, 70, 60
    images = eval_case_dense(7, 4, C, M, n_det, cls=3)
    rs = np.random.RandomState(3)
    for im in images:
        gc = im['gt_classes']
        gc[rs.permutation(M)[:20]] = rs.choice([0, C + 1, -1, -7, 1], 20)
    assert any((np.asarray(im['det_classes']) == v).any() for im in images for v in (0, C + 1, -3))
    ev = _evaluator(C)
    counts = [n_det + 50, 0, n_det, 7]                                         # max_det = n_det: clamped; none; all; a few
    tp, _ = _check_batch(ev, images, C, n_det, M, counts=counts)
    assert (tp[1] == -1).all() and (tp[3, 7:] == -1).all() and (tp[0] >= 0).any()
    _check_metrics(ev, images, C, ns=[n_det, 0, n_det, 7])


def test_eval_match_rejects_what_it_cannot_hold():
    import _hip
    from ood_object_detection_amd import _lib
    lib = _lib.load()
    z = torch.zeros(64, dtype=torch.int32, device=DEV)
    f = torch.zeros(64, device=DEV)
    l = torch.zeros(64, dtype=torch.int64, device=DEV)
    call = lambda B, max_det, M, C: lib.effdet_eval_match(_hip.stream(DEV), f.data_ptr(), z.data_ptr(), f.data_ptr(), l.data_ptr(), B,
                                                          max_det, M, C, 0.5, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr())
    assert call(1, 1, 0, 1) == -22 and call(0, 1, 1, 1) == -22 and call(1, 0, 1, 1) == -22 and call(1, 1, 1, 0) == -22
    assert call(1, 1, 9000, 1) == -22                                          # LDS: (C + 2 M + 8) ints must fit in 64 KiB


# ------------------------------------------------------------------------------------------------ average precision
def _eval_ap(scores, classes, tp, gt_count, C, short=0):
    import _hip
    from ood_object_detection_amd import _lib
    lib = _lib.load()
    n = len(scores)
    s = torch.from_numpy(np.asarray(scores, np.float32)).to(DEV)
    c = torch.from_numpy(np.asarray(classes, np.int32)).to(DEV)
    t = torch.from_numpy(np.asarray(tp, np.int32)).to(DEV)
    g = torch.from_numpy(np.asarray(gt_count, np.int32)).to(DEV)
    ap = torch.full((C,), 123.0, dtype=torch.float64, device=DEV)
    nb = lib.effdet_eval_ap_workspace_bytes(n)
    ws = torch.empty((nb + 7) // 8, dtype=torch.float64, device=DEV)
    rc = lib.effdet_eval_ap(_hip.stream(DEV), s.data_ptr(), c.data_ptr(), t.data_ptr(), n, C, g.data_ptr(), ap.data_ptr(), ws.data_ptr(),
                            nb - short)
    torch.cuda.synchronize()
    return rc, ap.cpu().numpy()


def _oracle_ap(scores, classes, tp, gt_count, C):
    scores, classes, tp = np.asarray(scores), np.asarray(classes), np.asarray(tp)
    out = np.full(C, np.nan)
    for c in range(C):
        sel = (classes == c) & (tp >= 0)
        out[c] = oe.average_precision(scores[sel], tp[sel], gt_count[c])
    return out


# n = 65 536 is the entry point's limit; its O(n^2) pair counting stays in the seconds on the device, so the size is kept
@pytest.mark.parametrize('n', [1, 255, 257, 20000, 65536])
def test_eval_ap_sizes_and_equal_scores(n):
    """scores quantised into blocks of equal values; inside a block of one class all flags are equal, so the result does not
    depend on the order of ties.  Class 0 has ground truth and no detection (AP 0), class 1 detections and no ground truth
    (NaN); rows with tp = -1 or class -1 are ignored."""
    C = 7
    rs = np.random.RandomState(n)
    classes = rs.choice([-1, 1, 2, 3, 4, 5, 6], n, p=[0.1, 0.1, 0.3, 0.2, 0.1, 0.1, 0.1])
    levels = max(2, n // 40)
    q = rs.randint(0, levels, n)
    scores = (q / float(levels)).astype(np.float32)
    flag = rs.randint(0, 2, (C + 1, levels))                                   # one flag per (class, score block)
    tp = flag[classes, q]
    tp[rs.uniform(size=n) < 0.1] = -1
    gt_count = np.array([5] + [0] + [int(((classes == c) & (tp > 0)).sum()) + rs.randint(0, 9) for c in range(2, C)])
    gt_count[6] = 0 if n == 257 else gt_count[6]
    rc, ap = _eval_ap(scores, classes, tp, gt_count, C)
    assert rc == 0
    ref = _oracle_ap(scores, classes, tp, gt_count, C)
    assert np.allclose(ap, ref, rtol=0, atol=1e-12, equal_nan=True), (ap, ref)
    assert ap[0] == 0.0 and np.isnan(ap[1])
    # order of the ties does not matter here: the same rows shuffled give the same AP
    perm = rs.permutation(n)
    rc, ap2 = _eval_ap(scores[perm], classes[perm], tp[perm], gt_count, C)
    assert rc == 0 and np.allclose(ap2, ref, rtol=0, atol=1e-12, equal_nan=True)


def test_eval_ap_equal_scores_with_mixed_flags_lower_index_first():
    """the documented rule: of equal scores the lower index ranks first.  FP, TP, TP at one score with 2 ground-truth boxes:
    precisions 0, 1/2, 2/3 -> AP 2/3; the opposite order would give 1."""
    s = [0.5, 0.9, 0.5, 0.5, 0.5, 0.1]
    c = [0, 1, 0, -1, 0, 0]
    tp = [0, 1, 1, 1, 1, -1]
    rc, ap = _eval_ap(s, c, tp, [2, 1], 2)
    assert rc == 0
    ref = _oracle_ap(s, c, tp, [2, 1], 2)
    assert abs(ref[0] - 2.0 / 3.0) < 1e-15 and ref[1] == 1.0
    assert np.allclose(ap, ref, rtol=0, atol=1e-12)
    rc, ap = _eval_ap(s, c, [1, 1, 1, 1, 0, -1], [2, 1], 2)                    # TP, TP, FP
    assert rc == 0 and abs(ap[0] - 1.0) < 1e-12


def test_eval_ap_rejects_bad_sizes():
    assert _eval_ap([0.5] * 10, [0] * 10, [1] * 10, [3], 1, short=1)[0] == -22
    from ood_object_detection_amd import _lib
    assert _lib.load().effdet_eval_ap_workspace_bytes(0) == -22


def test_evaluator_equal_scores_across_images():
    """through the evaluator: equal scores inside an image and across images; per class the order is (image, position)"""
    C = 3
    gt = np.array([[0, 0, 10, 10], [30, 30, 40, 40]], np.float32)
    mk = lambda boxes, cls: dict(gt_boxes=gt, gt_classes=np.array([1, 1]), det_boxes=np.array(boxes, np.float32),
                                 det_scores=np.full(len(boxes), 0.5, np.float32), det_classes=np.array(cls))
    images = [mk([[50, 50, 60, 60], [0, 0, 10, 10], [0, 0, 10, 10]], [1, 1, 1]),           # FP, TP, FP (taken)
              mk([[30, 30, 40, 40], [70, 70, 80, 80]], [1, 2]),                              # TP; class 2 without ground truth
              mk([[0, 0, 10, 10], [30, 30, 40, 40]], [1, 1])]                                # TP, TP
    ev = _evaluator(C)
    for im in images:
        ev.add_single_ground_truth_image_info(len(ev._image_ids), {'bbox': im['gt_boxes'], 'cls': im['gt_classes']})
    for i, im in enumerate(images):
        ev.add_single_detected_image_info(i, {'bbox': im['det_boxes'], 'scores': im['det_scores'], 'cls': im['det_classes']})
    ap = _check_metrics(ev, images, C)
    # FP TP FP TP TP TP over 6 ground-truth boxes: envelope 2/3 at all four true positives -> AP = 4/6 * 2/3
    assert abs(ap[0] - 4.0 / 9.0) < 1e-12 and np.isnan(ap[1]) and np.isnan(ap[2])
