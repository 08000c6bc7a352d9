"""numpy restatement of the open-set detection evaluation (csrc/eval_scale.hip, effdet/evaluation/open_set_evaluator.py), written
the slow, obvious way.  Test infrastructure only.

Classes are 0-based here as in tests/_eval_scale_ref.py: known classes 0 .. C-1, the unknown class is C (1-based: U = C + 1).
  matching      _eval_scale_ref.match_image with C + 1 classes: the unknown class is matched like any other
  open word     bit t of a kept detection of a known class = the largest IoU between its box and the image's ground-truth boxes of
                class C (difficult or not) is >= thresholds[t]; IoU in float32, the kernel's operations in the kernel's order
  counts        per (threshold, class) over the class's kept entries in the sorted order (score descending, ties by arrival):
                n_det, tp, open_total, and where the class has ground truth and an entry: pos = OWOD's
                min(range(len(rec)), key=lambda i: abs(rec[i] - level)), k_star = ctp[pos], rank_at, open_at
  metrics       float64 from the integers
"""
import numpy as np

import _eval_scale_ref as R

INVALID = R.INVALID
MATRICES = ('n_det', 'tp', 'open_total', 'k_star', 'pos', 'rank_at', 'open_at')


def iou32(d, g):
    """d: one detection box yxyx, g: [k, 4] ground-truth boxes yxyx -> [k] float32 IoU, inter / (area_d + area_g - inter) with the
    operations of es_match_kernel in its order (every numpy operation on float32 arrays rounds once, like the kernel's)"""
    d, g = np.asarray(d, np.float32), np.asarray(g, np.float32).reshape(-1, 4)
    zero = np.float32(0)
    with np.errstate(all='ignore'):
        area_d = (d[2] - d[0]) * (d[3] - d[1])
        ih = np.maximum(zero, np.minimum(d[2], g[:, 2]) - np.maximum(d[0], g[:, 0]))
        iw = np.maximum(zero, np.minimum(d[3], g[:, 3]) - np.maximum(d[1], g[:, 1]))
        inter = ih * iw
        area_g = (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1])
        iou = inter / (area_d + area_g - inter)
    assert iou.dtype == np.float32
    return iou


def open_words_image(im, num_known, thresholds, flags):
    """[n] uint32 open words of one image (layout of _eval_scale_ref.match_image, unknown class = num_known)"""
    det_boxes = np.asarray(im['det_boxes'], np.float32).reshape(-1, 4)
    det_classes = np.asarray(im['det_classes']).reshape(-1)
    gt_boxes = np.asarray(im['gt_boxes'], np.float32).reshape(-1, 4)
    gt_classes = np.asarray(im['gt_classes']).reshape(-1)
    words = np.zeros(len(det_classes), np.uint32)
    unknown = gt_boxes[gt_classes == num_known]
    for i in range(len(det_classes)):
        if (flags[i] & INVALID) or not 0 <= det_classes[i] < num_known:
            continue
        best = np.float32(-np.inf)
        for iou in iou32(det_boxes[i], unknown):
            if iou > best:                                                    # a NaN never wins
                best = iou
        for t, thr in enumerate(thresholds):
            if best >= np.float32(thr):
                words[i] |= np.uint32(1 << t)
    return words


def sorted_order(scores, classes, flags, num_classes):
    """indices of the valid entries in the device's order: class, then score descending, equal scores (-0.0 == +0.0) by arrival"""
    scores, classes, flags = np.asarray(scores, np.float32), np.asarray(classes), np.asarray(flags, np.uint32)
    ok = np.nonzero(((flags & INVALID) == 0) & (classes >= 0) & (classes < num_classes) & ~np.isnan(scores))[0]
    ok = ok[np.argsort(-scores[ok], kind='stable')]
    return ok[np.argsort(classes[ok], kind='stable')]


def brute_force_position(ctp, n_gt, level):
    """OWOD: the first position whose recall is nearest the level (float64)"""
    rec = [np.float64(k) / np.float64(n_gt) for k in ctp]
    return min(range(len(rec)), key=lambda i: abs(rec[i] - np.float64(level)))


def counts_from_entries(scores, classes, flags, words, gt_count, num_classes, T, level):
    """the seven int64 matrices [T, num_classes] over accumulated entries in arrival order"""
    flags, words, classes = np.asarray(flags, np.uint32), np.asarray(words, np.uint32), np.asarray(classes)
    order = sorted_order(scores, classes, flags, num_classes)
    out = {k: np.zeros((T, num_classes), np.int64) for k in MATRICES}
    out['pos'][:] = -1
    for c in range(num_classes):
        seg = order[classes[order] == c]
        for t in range(T):
            ni = [int(not (int(flags[i]) >> (16 + t)) & 1) for i in seg]
            tp = [(int(flags[i]) >> t) & 1 for i in seg]
            op = [(int(words[i]) >> t) & 1 for i in seg]
            out['n_det'][t, c], out['tp'][t, c], out['open_total'][t, c] = sum(ni), sum(tp), sum(op)
            if gt_count[c] > 0 and len(seg) > 0:
                ctp = np.cumsum(tp)
                pos = brute_force_position(ctp, gt_count[c], level)
                out['pos'][t, c], out['k_star'][t, c] = pos, ctp[pos]
                out['rank_at'][t, c], out['open_at'][t, c] = sum(ni[:pos + 1]), sum(op[:pos + 1])
    return out


def metrics(r, num_known):
    """float64 metrics from the integer matrices and gt_count / ap of `r`"""
    T, C = r['tp'].shape[0], num_known
    nan = float('nan')
    div = lambda a, b: float(a) / float(b) if b != 0 else (nan if a == 0 else float('inf'))
    out = dict(recall=np.array([[div(r['tp'][t, c], r['gt_count'][c]) for c in range(C + 1)] for t in range(T)]),
               precision=np.array([[div(r['tp'][t, c], r['n_det'][t, c]) for c in range(C + 1)] for t in range(T)]),
               precision_at_recall=np.array([[div(r['k_star'][t, c], r['rank_at'][t, c]) for c in range(C + 1)] for t in range(T)]))
    out['a_ose'] = np.array([sum(int(r['open_total'][t, c]) for c in range(C)) for t in range(T)])
    wi = []
    for t in range(T):
        s = [c for c in range(C) if r['gt_count'][c] > 0 and r['pos'][t, c] >= 0]
        num, den = sum(int(r['open_at'][t, c]) for c in s), sum(int(r['rank_at'][t, c]) for c in s)
        wi.append(num / den if s and den else nan)
    out['wi'] = np.array(wi)
    out['u_recall'], out['u_precision'], out['u_ap'] = out['recall'][:, C], out['precision'][:, C], r['ap'][:, C]
    return out


def evaluate(images, num_known, thresholds=(0.5,), level=0.8):
    """images as in _eval_scale_ref.match_image with classes 0 .. num_known (num_known = unknown).  -> the dict of
    _eval_scale_ref.evaluate over num_known + 1 classes, `open` (arrival order), the seven matrices and the metrics"""
    r = R.evaluate(images, num_known + 1, thresholds)
    words, k = [], 0
    for im in images:
        n = len(np.asarray(im['det_scores']).reshape(-1))
        words.append(open_words_image(im, num_known, thresholds, r['flags'][k:k + n]))
        k += n
    r['open'] = np.concatenate(words) if words else np.zeros(0, np.uint32)
    r.update(counts_from_entries(r['scores'], r['classes'], r['flags'], r['open'], r['gt_count'], num_known + 1, len(thresholds), level))
    r.update(metrics(r, num_known))
    return r


# ------------------------------------------------------------------------------------------------ seeded cases shared by the tests
CASE_THRESHOLDS = (0.25, 0.5, 0.9)


def open_case(seed, n_img, n_det, C, M, n_unknown):
    """0-based images for `evaluate` with unknown class C: M ground-truth boxes, 10 x 10 on a 30-pixel integer grid with duplicates
    (IoU ties, also between unknown boxes; box 1 repeats box 0 with another class: a detection on it overlaps a known and an
    unknown box), `n_unknown` of them unknown, some difficult (unknown ones too), two degenerate.  Image 1 has no ground truth,
    image 2 no detections, image 3 only unknown ground truth.  Detections, scores descending: exact copies of ground-truth boxes,
    integer boxes at IoU exactly 0.5 (10 x 20 on 10 x 10) and exactly 0.25 (10 x 40), random and degenerate boxes, NaN scores,
    classes known, unknown and outside 0..C."""
    rs = np.random.RandomState(seed)
    images = []
    for b in range(n_img):
        k = np.arange(M)
        gt = np.stack([30.0 * (k // 20), 30.0 * (k % 20), 30.0 * (k // 20) + 10, 30.0 * (k % 20) + 10], 1).astype(np.float32)
        for j in range(1, M):
            if rs.uniform() < 1.0 / 6:
                gt[j] = gt[j - 1]
        gc = rs.randint(0, C, M)
        unk = rs.permutation(M)[:min(n_unknown, M)]
        gc[unk] = C
        if M >= 2 and n_unknown >= 1:
            gt[1] = gt[0]
            gc[0], gc[1] = C, 0
        if M >= 8:
            gt[5] = gt[5][[2, 1, 0, 3]] + np.array([0, 0, 2.5, 0.25], np.float32)   # ymax < ymin; no integer box makes the union 0
            gt[6, 3] = gt[6, 1]                                               # zero width
        if b == 1:
            gc[:] = -1
        if b == 3:
            gc[:] = C
        dif = rs.uniform(size=M) < 0.2
        n = 0 if b == 2 else n_det
        det, dc = [], []
        for _ in range(n):
            r, j = rs.uniform(), rs.randint(0, M)
            if r < 0.3:
                box = gt[j].copy()
            elif r < 0.5:
                box = gt[j] + np.array([0, 0, 0, 10], np.float32)
            elif r < 0.65:
                box = gt[j] + np.array([0, 0, 0, 30], np.float32)
            elif r < 0.9:
                yy, xx = np.floor(rs.uniform(0, 60)), np.floor(rs.uniform(0, 560))
                box = np.array([yy, xx, yy + np.floor(rs.uniform(5, 40)), xx + np.floor(rs.uniform(5, 40))], np.float32)
            else:
                box = np.array([7, 7, 3, 12], np.float32)                     # ymax < ymin
            det.append(box)
            u = rs.uniform()
            dc.append(C if u < 0.2 else (-1 if u < 0.24 else (C + 1 if u < 0.28 else (gc[j] if u < 0.7 and gc[j] >= 0 else rs.randint(0, C)))))
        sc = np.sort(rs.permutation(100000)[:n].astype(np.float32) / np.float32(100000))[::-1].copy()
        if n > 10:
            sc[[3, n - 2]] = np.nan
        images.append(dict(gt_boxes=gt, gt_classes=np.asarray(gc, np.int64), gt_difficult=dif,
                           det_boxes=np.asarray(det, np.float32).reshape(-1, 4), det_scores=sc, det_classes=np.asarray(dc, np.int64)))
    return images


def pack(images, max_det, M):
    """0-based images -> numpy det [B,max_det,6] x1,y1,x2,y2,score,class (1-based), count [B] int32, gt_boxes [B,M,4], gt_cls [B,M]
    int64 (1-based, -1 padding), gt_difficult [B,M] uint8: the arguments of `add_batch`"""
    B = len(images)
    det, cnt = np.zeros((B, max_det, 6), np.float32), np.zeros(B, np.int32)
    gtb, gtc, gtd = np.zeros((B, M, 4), np.float32), np.full((B, M), -1, np.int64), np.zeros((B, M), np.uint8)
    for i, im in enumerate(images):
        n, m = len(im['det_scores']), len(im['gt_classes'])
        b = np.asarray(im['det_boxes'], np.float32).reshape(-1, 4)
        det[i, :n] = np.stack([b[:, 1], b[:, 0], b[:, 3], b[:, 2], np.asarray(im['det_scores'], np.float32),
                               (np.asarray(im['det_classes']) + 1).astype(np.float32)], 1)
        cnt[i] = n
        gtb[i, :m] = np.asarray(im['gt_boxes'], np.float32).reshape(-1, 4)
        gc = np.asarray(im['gt_classes'], np.int64)
        gtc[i, :m] = np.where(gc >= 0, gc + 1, -1)
        if 'gt_difficult' in im:
            gtd[i, :m] = np.asarray(im['gt_difficult']).astype(np.uint8)
    return det, cnt, gtb, gtc, gtd
