"""numpy restatement of the dataset-scale detection evaluation (csrc/eval_scale.hip): oracle/evaluation.py with `difficult`
ground truth and a list of IoU thresholds.  Test infrastructure only.

Follows, by reference file:line
  effdet/evaluation/per_image_evaluation.py:391-407  a detection's candidate is the ground-truth box of its class with the largest
                                                     IoU (first on ties, difficult boxes included); IoU >= threshold and the
                                                     candidate difficult -> the detection is ignored (:471 drops it); candidate
                                                     not taken -> true positive and taken; otherwise false positive
  effdet/evaluation/per_image_evaluation.py:143-176  CorLoc looks at every ground-truth box of the class, difficult or not
  effdet/evaluation/object_detection_evaluation.py:132-139  instances = boxes that are not difficult; an image counts for a class
                                                     as soon as the class occurs in it
The candidate does not depend on the threshold, so one flag word per detection describes all thresholds: bit t = true positive
at thresholds[t], bit 16 + t = ignored there, bit 31 = invalid (degenerate box, class outside 0..C-1, NaN score).

Equal scores: stable descending order, as oracle/evaluation.py documents.  IoU is oracle.evaluation.iou_matrix (float32).
Pinned to the reference's own evaluator by tests/golden/evaluation_scale.npz (tests/test_eval_scale_host.py).
"""
import numpy as np

from oracle.evaluation import average_precision, iou_matrix

INVALID = np.uint32(1 << 31)


def match_image(im, num_classes, thresholds):
    """im: dict(det_boxes yxyx, det_scores, det_classes, gt_boxes, gt_classes[, gt_difficult]), 0-based classes.
    -> (flag word per detection in the given order [n] uint32, correct [T, C] int)"""
    T = len(thresholds)
    thr = [np.float32(t) for t in thresholds]
    det_boxes = np.asarray(im['det_boxes'], np.float32).reshape(-1, 4)
    det_scores = np.asarray(im['det_scores'], np.float32).reshape(-1)
    det_classes = np.asarray(im['det_classes']).reshape(-1)
    gt_boxes = np.asarray(im['gt_boxes'], np.float32).reshape(-1, 4)
    gt_classes = np.asarray(im['gt_classes']).reshape(-1)
    difficult = np.asarray(im.get('gt_difficult', np.zeros(len(gt_classes))), bool).reshape(-1)
    valid = (det_boxes[:, 0] < det_boxes[:, 2]) & (det_boxes[:, 1] < det_boxes[:, 3]) & (det_classes >= 0) \
        & (det_classes < num_classes) & ~np.isnan(det_scores)
    flags = np.where(valid, np.uint32(0), INVALID).astype(np.uint32)
    correct = np.zeros((T, num_classes), dtype=np.int64)
    for c in range(num_classes):
        idx = np.nonzero(valid & (det_classes == c))[0]
        g = np.nonzero(gt_classes == c)[0]
        if idx.size == 0 or g.size == 0:
            continue
        idx = idx[np.argsort(-det_scores[idx], kind='stable')]
        iou = iou_matrix(det_boxes[idx], gt_boxes[g])
        best = np.argmax(iou, axis=1)
        for t in range(T):
            if iou[0, best[0]] >= thr[t]:                                   # the top-scoring detection of the class
                correct[t, c] = 1
        taken = np.zeros((T, g.size), bool)
        for k, i in enumerate(idx):
            j = best[k]
            for t in range(T):
                if not iou[k, j] >= thr[t]:
                    continue
                if difficult[g[j]]:
                    flags[i] |= np.uint32(1 << (16 + t))
                elif not taken[t, j]:
                    flags[i] |= np.uint32(1 << t)
                    taken[t, j] = True
    return flags, correct


def ap_from_entries(scores, classes, flags, gt_count, num_classes, T):
    """[T, C] VOC all-points AP over accumulated entries in arrival order; invalid entries take no part"""
    scores, classes, flags = np.asarray(scores, np.float32), np.asarray(classes), np.asarray(flags, np.uint32)
    ok = ((flags & INVALID) == 0) & (classes >= 0) & (classes < num_classes) & ~np.isnan(scores)
    ap = np.full((T, num_classes), np.nan)
    for c in range(num_classes):
        if gt_count[c] == 0:
            continue
        sel = ok & (classes == c)
        for t in range(T):
            use = sel & ((flags >> np.uint32(16 + t)) & 1 == 0)
            ap[t, c] = average_precision(scores[use], ((flags[use] >> np.uint32(t)) & 1).astype(bool), gt_count[c])
    return ap


def sorted_entries(scores, classes, flags, num_classes):
    """the device's order of the valid entries: class, then score descending, equal scores (-0.0 == +0.0) by arrival"""
    scores, classes, flags = np.asarray(scores, np.float32), np.asarray(classes), np.asarray(flags, np.uint32)
    ok = np.nonzero(((flags & INVALID) == 0) & (classes >= 0) & (classes < num_classes) & ~np.isnan(scores))[0]
    ok = ok[np.argsort(-scores[ok], kind='stable')]
    ok = ok[np.argsort(classes[ok], kind='stable')]
    return classes[ok].astype(np.int64), scores[ok] + np.float32(0), flags[ok]


def evaluate(images, num_classes, thresholds=(0.5,)):
    """images as in match_image.  -> dict(ap [T, C], corloc [T, C], mean_ap [T], mean_corloc [T], gt_count, gt_imgs, correct,
    scores / classes / flags: the accumulated entries in (image, position) order, invalid ones included)"""
    T = len(thresholds)
    gt_count = np.zeros(num_classes, np.int64)
    gt_imgs = np.zeros(num_classes, np.int64)
    correct = np.zeros((T, num_classes), np.int64)
    scores, classes, flags = [], [], []
    for im in images:
        gc = np.asarray(im['gt_classes']).reshape(-1)
        difficult = np.asarray(im.get('gt_difficult', np.zeros(len(gc))), bool).reshape(-1)
        for c in range(num_classes):
            gt_count[c] += int(np.sum((gc == c) & ~difficult))
            gt_imgs[c] += 1 if np.any(gc == c) else 0
        f, cor = match_image(im, num_classes, thresholds)
        correct += cor
        scores.append(np.asarray(im['det_scores'], np.float32).reshape(-1))
        classes.append(np.asarray(im['det_classes'], np.int64).reshape(-1))
        flags.append(f)
    scores = np.concatenate(scores) if scores else np.zeros(0, np.float32)
    classes = np.concatenate(classes) if classes else np.zeros(0, np.int64)
    flags = np.concatenate(flags) if flags else np.zeros(0, np.uint32)
    ap = ap_from_entries(scores, classes, flags, gt_count, num_classes, T)
    with np.errstate(invalid='ignore', divide='ignore'):
        corloc = np.where(gt_imgs[None] == 0, np.nan, correct / gt_imgs[None].astype(float))
        mean_ap = np.array([np.nanmean(ap[t]) if np.isfinite(ap[t]).any() else np.nan for t in range(T)])
        mean_corloc = np.array([np.nanmean(corloc[t]) if np.isfinite(corloc[t]).any() else np.nan for t in range(T)])
    return dict(ap=ap, corloc=corloc, mean_ap=mean_ap, mean_corloc=mean_corloc, gt_count=gt_count, gt_imgs=gt_imgs,
                correct=correct, scores=scores, classes=classes, flags=flags)


def zero_based(im, difficult=None):
    """an image of tests/_seeded.py::eval_case (1-based classes) in the layout of match_image"""
    out = dict(det_boxes=im['det_boxes'], det_scores=im['det_scores'], det_classes=np.asarray(im['det_classes']) - 1,
               gt_boxes=im['gt_boxes'], gt_classes=np.asarray(im['gt_classes']) - 1)
    if difficult is not None:
        out['gt_difficult'] = np.asarray(difficult, bool)
    elif 'gt_difficult' in im:
        out['gt_difficult'] = np.asarray(im['gt_difficult'], bool)
    return out


def fixture_case(g, tag):
    """(images with the fixture's difficult flags, 0-based; C) of case `tag` of tests/golden/evaluation_scale.npz"""
    from _seeded import eval_case
    seed, n_img, C, n_det = [int(v) for v in g[tag + '_meta']]
    images = eval_case(seed, n_img, C, n_det)
    d = g[tag + '_difficult'].astype(bool)
    out, k = [], 0
    for im in images:
        m = len(im['gt_classes'])
        out.append(zero_based(im, d[k:k + m]))
        k += m
    assert k == len(d)
    return out, C
