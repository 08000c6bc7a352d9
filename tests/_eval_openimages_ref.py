"""numpy restatement of the OpenImages detection evaluation (csrc/openimages_eval.hip): tests/_eval_scale_ref.py with group-of
boxes, their weight, the Challenge's verified image-level labels and the pooled ("weighted") mean AP.  Test infrastructure only.

Follows, by reference file:line
  effdet/evaluation/per_image_evaluation.py:297-300  IoU against the boxes that are not group-of, IoA (intersection over the
                                                     DETECTION's area, np_box_ops.ioa) against the group-of boxes
  effdet/evaluation/per_image_evaluation.py:391-407  stage 1: the candidate is the box with the largest IoU (first on ties,
                                                     difficult boxes included); IoU >= thr and difficult -> ignored; not taken
                                                     -> true positive and taken; otherwise, so far, a false positive
  effdet/evaluation/per_image_evaluation.py:423-434  stage 2: a detection that is neither takes the group-of box with the largest
                                                     IoA (first on ties); IoA >= thr -> absorbed, the box keeps the largest score
  effdet/evaluation/per_image_evaluation.py:435-437  a box with a kept score > 0 gives one entry of weight w when w > 0
  effdet/evaluation/per_image_evaluation.py:471-473  ignored and absorbed detections leave; the virtual entries follow the rest
  effdet/evaluation/per_image_evaluation.py:143-176  CorLoc: the top-scoring detection against every box of the class by IoU
  effdet/evaluation/object_detection_evaluation.py:132-139  num_gt = (not difficult, not group-of) + w (group-of, not difficult)
  effdet/evaluation/object_detection_evaluation.py:221-264  pooled AP: the entries of all classes with num_gt > 0, num_gt summed
  effdet/evaluation/detection_evaluator.py:536-544, 568-572  Challenge: detections of classes outside (box classes + labels) leave
  effdet/evaluation/metrics.py:36-44, 80-88          precision = ctp / (ctp + cfp), recall = ctp / num_gt, VOC all-points AP

Stage-1 and stage-2 candidates do not depend on the threshold, so one flag word per detection describes all T <= 15 thresholds:
bit t = true positive at thresholds[t], bit 16 + t = ignored or absorbed there, bit 31 = dropped.  A virtual entry is per (box,
threshold): bit t | the ignore bits of every other threshold | bit 15.  Detections are walked in the order given (the device
takes rows in descending score order).  A box that is both difficult and group-of absorbs and is counted nowhere (the reference
is ill-defined there).

`ap_segment` adds in the kernel's order - 2048-entry chunks from the last to the first, eight entries a thread, a butterfly over
the 64 lanes of a wave, the four waves in ascending order - so its result is compared bitwise with the device's.  Against the
reference's fixture the same terms are added in the reference's order (`reference_order`): the order of a float64 sum shows in its
last bit, and only that differs between the two.
"""
import numpy as np

from oracle.evaluation import iou_matrix

INVALID = np.uint32(1 << 31)
GROUP = np.uint32(1 << 15)
CHUNK, ITEMS, WAVE = 2048, 8, 64


def ioa_matrix(det, gt):
    """det [N,4], gt [M,4] yxyx float32 -> [N,M] float32: intersection over the detection's area (np_box_ops.ioa, transposed)"""
    a, b = np.asarray(det, np.float32).reshape(-1, 4), np.asarray(gt, np.float32).reshape(-1, 4)
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    ih = np.maximum(np.float32(0), np.minimum(a[:, 2:3], b[:, 2][None]) - np.maximum(a[:, 0:1], b[:, 0][None]))
    iw = np.maximum(np.float32(0), np.minimum(a[:, 3:4], b[:, 3][None]) - np.maximum(a[:, 1:2], b[:, 1][None]))
    with np.errstate(all='ignore'):
        return (ih * iw) / area_a[:, None]


def _flags_of(im, key, m):
    return np.asarray(im.get(key, np.zeros(m)), bool).reshape(-1)


def match_image(im, num_classes, thresholds, emit=True):
    """im: dict(det_boxes yxyx, det_scores, det_classes, gt_boxes, gt_classes[, gt_difficult, gt_group_of, labeled_cls]), 0-based
    classes; labeled_cls None / absent: every class is evaluatable.
    -> (flag word per detection [n] uint32, vscore [m, T] float32, vflags [m, T] uint32, correct [T, C] int)"""
    T = len(thresholds)
    assert 1 <= T <= 15
    thr = [np.float32(t) for t in thresholds]
    det_boxes = np.asarray(im['det_boxes'], np.float32).reshape(-1, 4)
    det_scores = np.asarray(im['det_scores'], np.float32).reshape(-1)
    det_classes = np.asarray(im['det_classes']).reshape(-1)
    gt_boxes = np.asarray(im['gt_boxes'], np.float32).reshape(-1, 4)
    gt_classes = np.asarray(im['gt_classes']).reshape(-1)
    m = len(gt_classes)
    difficult, group = _flags_of(im, 'gt_difficult', m), _flags_of(im, 'gt_group_of', m)
    valid = (det_boxes[:, 0] < det_boxes[:, 2]) & (det_boxes[:, 1] < det_boxes[:, 3]) & (det_classes >= 0) \
        & (det_classes < num_classes) & ~np.isnan(det_scores)
    if im.get('labeled_cls') is not None:
        allowed = set(int(c) for c in gt_classes if 0 <= c < num_classes) | set(int(c) for c in np.asarray(im['labeled_cls']).reshape(-1))
        valid &= np.array([int(c) in allowed for c in det_classes], bool).reshape(-1)
    flags = np.where(valid, np.uint32(0), INVALID).astype(np.uint32)
    gscore = np.zeros((m, T), np.float32)
    correct = np.zeros((T, num_classes), dtype=np.int64)
    with np.errstate(all='ignore'):
        iou = iou_matrix(det_boxes, gt_boxes) if m and len(det_boxes) else np.zeros((len(det_boxes), m), np.float32)
    ioa = ioa_matrix(det_boxes, gt_boxes) if m and len(det_boxes) else np.zeros((len(det_boxes), m), np.float32)
    all_bits = (1 << T) - 1
    for c in range(num_classes):
        idx = np.nonzero(valid & (det_classes == c))[0]
        g = np.nonzero((gt_classes == c))[0]
        if idx.size == 0 or g.size == 0:
            continue
        plain, grp = g[~group[g]], g[group[g]]
        top = iou[idx[0], g].max()
        for t in range(T):
            if top >= thr[t]:                                               # the top-scoring detection against EVERY box
                correct[t, c] = 1
        taken = np.zeros((T, m), bool)
        for i in idx:
            tp = ign = 0
            if plain.size:
                j = plain[np.argmax(iou[i, plain])]
                for t in range(T):
                    if not iou[i, j] >= thr[t]:
                        continue
                    if difficult[j]:
                        ign |= 1 << t
                    elif not taken[t, j]:
                        tp |= 1 << t
                        taken[t, j] = True
            absorbed = 0
            if grp.size:
                j = grp[np.argmax(ioa[i, grp])]
                for t in range(T):
                    if ioa[i, j] >= thr[t] and not ((tp | ign) >> t) & 1:
                        absorbed |= 1 << t
                        gscore[j, t] = max(gscore[j, t], det_scores[i])
            flags[i] = np.uint32(tp | ((ign | absorbed) << 16))
    vscore = np.zeros((m, T), np.float32)
    vflags = np.full((m, T), INVALID, np.uint32)
    if emit:
        for j in range(m):
            if not group[j] or not 0 <= gt_classes[j] < num_classes:
                continue
            for t in range(T):
                if gscore[j, t] > 0:
                    vscore[j, t] = gscore[j, t]
                    vflags[j, t] = np.uint32((1 << t) | ((all_bits & ~(1 << t)) << 16)) | GROUP
    return flags, vscore, vflags, correct


def num_gt(n_plain, n_group, w):
    return np.asarray(n_plain, np.float64) + np.float64(w) * np.asarray(n_group, np.float64)


def ap_segment(flags, t, w, ngt, reference_order=False):
    """the weighted VOC AP at threshold t of one sorted segment.  The terms - one per true positive, (recall step) * (envelope of
    precision) - are the same either way; they are added in the kernel's order, or with reference_order as metrics.py:88 adds
    them (np.sum over the true positives' terms), which can differ in the last bit."""
    f = np.asarray(flags, np.uint32).astype(np.int64)
    n = len(f)
    if n == 0:
        return 0.0
    w, ngt = np.float64(w), np.float64(ngt)
    ni = ((f >> (16 + t)) & 1) == 0
    tp = ((f >> t) & 1) == 1
    grp = ((f >> 15) & 1) == 1
    ai, gi = (tp & ~grp).astype(np.int64), (tp & grp).astype(np.int64)
    rank, a, g = np.cumsum(ni.astype(np.int64)), np.cumsum(ai), np.cumsum(gi)
    before = (a - ai).astype(np.float64) + w * (g - gi).astype(np.float64)
    ctp = a.astype(np.float64) + w * g.astype(np.float64)
    with np.errstate(all='ignore'):
        prec = np.where(ni, ctp / (ctp + (rank - a - g).astype(np.float64)), 0.0)
        step = np.where(tp, ctp / ngt - before / ngt, 0.0)
    env = np.fmax.accumulate(prec[::-1])[::-1]
    term = np.where(tp, step * env, 0.0)
    if reference_order:
        return float(np.sum(term[tp]))
    chunks = (n + CHUNK - 1) // CHUNK
    x = np.zeros(chunks * CHUNK, np.float64)
    x[:n] = term
    x = x.reshape(chunks, CHUNK // ITEMS // WAVE, WAVE, ITEMS)
    s = np.zeros(x.shape[:3], np.float64)
    for r in range(ITEMS):
        s = s + x[..., r]
    lane = np.arange(WAVE)
    o = WAVE // 2
    while o:
        s = s + s[..., lane ^ o]
        o //= 2
    tot = s[:, 0, 0]
    for k in range(1, s.shape[1]):
        tot = tot + s[:, k, 0]
    acc = np.float64(0.0)
    for q in range(chunks - 1, -1, -1):
        acc = acc + tot[q]
    return float(acc)


def sorted_entries(scores, classes, flags, num_classes):
    """the device's order of the valid entries: class, then score descending, equal scores (-0.0 == +0.0) by arrival"""
    scores, classes, flags = np.asarray(scores, np.float32), np.asarray(classes), np.asarray(flags, np.uint32)
    ok = np.nonzero(((flags & INVALID) == 0) & (classes >= 0) & (classes < num_classes) & ~np.isnan(scores))[0]
    ok = ok[np.argsort(-scores[ok], kind='stable')]
    ok = ok[np.argsort(classes[ok], kind='stable')]
    return classes[ok].astype(np.int64), scores[ok] + np.float32(0), flags[ok]


def pooled_entries(cls, sc, fl, n_plain, n_group, w):
    """the class-sorted entries -> those of the classes with instances by score descending, equal scores by (class, arrival)"""
    has = num_gt(n_plain, n_group, w) > 0
    sel = np.nonzero(has[cls])[0] if len(cls) else np.zeros(0, np.int64)
    sel = sel[np.argsort(-sc[sel], kind='stable')]
    return cls[sel], sc[sel], fl[sel]


def ap_from_entries(scores, classes, flags, n_plain, n_group, w, num_classes, T, pooled=True, reference_order=False):
    """-> dict(ap [T, C], pooled_ap [T], sorted: (cls, score, flags), pooled: (cls, score, flags))"""
    cls, sc, fl = sorted_entries(scores, classes, flags, num_classes)
    ngt = num_gt(n_plain, n_group, w)
    ap = np.full((T, num_classes), np.nan)
    for c in range(num_classes):
        if not ngt[c] > 0:
            continue
        seg = fl[cls == c]
        for t in range(T):
            ap[t, c] = ap_segment(seg, t, w, ngt[c], reference_order)
    pooled_ap = np.full(T, np.nan)
    pe = pooled_entries(cls, sc, fl, n_plain, n_group, w)
    if pooled:
        has = ngt > 0
        total = np.float64(np.asarray(n_plain, np.int64)[has].sum()) + np.float64(w) * np.float64(np.asarray(n_group, np.int64)[has].sum())
        if total > 0:
            for t in range(T):
                pooled_ap[t] = ap_segment(pe[2], t, w, total, reference_order)
    return dict(ap=ap, pooled_ap=pooled_ap, sorted=(cls, sc, fl), pooled=pe)


def evaluate(images, num_classes, thresholds=(0.5,), w=0.0, pooled=True, reference_order=False):
    """images as in match_image; reference_order: see ap_segment.  -> dict(ap [T, C], pooled_ap [T], corloc [T, C], n_plain, n_group, gt_imgs, correct, flags /
    vscore / vflags: per image, scores / classes / words: the accumulated entries in append order (per image its detection rows,
    dropped ones included, then its virtual entries in (box, threshold) order), sorted, pooled)"""
    T = len(thresholds)
    n_plain = np.zeros(num_classes, np.int64)
    n_group = np.zeros(num_classes, np.int64)
    gt_imgs = np.zeros(num_classes, np.int64)
    correct = np.zeros((T, num_classes), np.int64)
    scores, classes, words, per_flags, per_vs, per_vf = [], [], [], [], [], []
    for im in images:
        gc = np.asarray(im['gt_classes']).reshape(-1)
        difficult, group = _flags_of(im, 'gt_difficult', len(gc)), _flags_of(im, 'gt_group_of', len(gc))
        for c in range(num_classes):
            n_plain[c] += int(np.sum((gc == c) & ~difficult & ~group))
            n_group[c] += int(np.sum((gc == c) & group & ~difficult))
            gt_imgs[c] += 1 if np.any(gc == c) else 0
        f, vs, vf, cor = match_image(im, num_classes, thresholds, emit=w > 0)
        correct += cor
        per_flags.append(f)
        per_vs.append(vs)
        per_vf.append(vf)
        live = (vf.reshape(-1) & INVALID) == 0
        scores += [np.asarray(im['det_scores'], np.float32).reshape(-1), vs.reshape(-1)[live]]
        classes += [np.asarray(im['det_classes'], np.int64).reshape(-1), np.repeat(gc.astype(np.int64), T)[live]]
        words += [f, vf.reshape(-1)[live]]
    scores = np.concatenate(scores) if scores else np.zeros(0, np.float32)
    classes = np.concatenate(classes) if classes else np.zeros(0, np.int64)
    words = np.concatenate(words) if words else np.zeros(0, np.uint32)
    out = ap_from_entries(scores, classes, words, n_plain, n_group, w, num_classes, T, pooled, reference_order)
    with np.errstate(invalid='ignore', divide='ignore'):
        corloc = np.where(gt_imgs[None] == 0, np.nan, correct / gt_imgs[None].astype(float))
    out.update(corloc=corloc, n_plain=n_plain, n_group=n_group, gt_imgs=gt_imgs, correct=correct, flags=per_flags, vscore=per_vs,
               vflags=per_vf, scores=scores, classes=classes, words=words)
    return out


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def dense_case(seed, n_img, C, M, n_det, group_frac, classes_used=2, difficult_frac=0.1, labels=None):
    """seeded inputs that fill the matching kernel: every image has exactly M boxes of the first `classes_used` classes, 10 x 10
    (group-of: 20 x 20) integer boxes on a 30-pixel grid, about one in six a duplicate of the box before it; group_frac of them
    group-of (0: none, 1: all), difficult_frac of the others difficult.  Detections in descending distinct scores, the last few
    <= 0: copies of a box (IoU 1, IoA 1), its left half (IoU exactly 0.5, IoA 1), the box widened to twice its width (IoU and IoA
    exactly 0.5), its top-left quarter (IoU 0.25, IoA 1), random boxes, degenerate boxes, classes outside 0..C-1 and other classes.
    labels: None, or the number of verified labels drawn per image (the Challenge list).  0-based classes."""
    rs = np.random.RandomState(seed)
    images = []
    for _ in range(n_img):
        group = rs.uniform(size=M) < group_frac
        difficult = (rs.uniform(size=M) < difficult_frac) & ~group
        gt = np.zeros((M, 4), np.float32)
        for k in range(M):
            if k > 0 and rs.uniform() < 1.0 / 6:
                gt[k] = gt[k - 1]
            else:
                y, x = 30.0 * (k // 20), 30.0 * (k % 20)
                side = 20 if group[k] else 10
                gt[k] = (y, x, y + side, x + side)
        gc = rs.randint(0, classes_used, M).astype(np.int64)
        det, dc = [], []
        for _k in range(n_det):
            r = rs.uniform()
            j = rs.randint(0, M)
            c = gc[j]
            y0, x0, y1, x1 = gt[j]
            if r < 0.3:
                box = gt[j].copy()
            elif r < 0.45:
                box = np.array([y0, x0, y1, x0 + (x1 - x0) / 2], np.float32)
            elif r < 0.6:
                box = np.array([y0, x0, y1, x1 + (x1 - x0)], np.float32)
            elif r < 0.7:
                box = np.array([y0, x0, y0 + (y1 - y0) / 2, x0 + (x1 - x0) / 2], np.float32)
            elif r < 0.82:
                yy, xx = rs.uniform(0, 400), rs.uniform(0, 560)
                box = np.array([yy, xx, yy + rs.uniform(5, 40), xx + rs.uniform(5, 40)], np.float32)
            elif r < 0.87:
                box = gt[j][[2, 1, 0, 3]].copy()                                         # degenerate: ymax < ymin
            else:
                box = gt[j].copy()
                c = [-1, C, -4, (c + 1) % C, C - 1][rs.randint(0, 5)]
            det.append(box)
            dc.append(c)
        sc = np.sort((rs.permutation(100000)[:n_det].astype(np.float32) - 3000) / 100000.0)[::-1].copy()
        im = dict(gt_boxes=gt, gt_classes=gc, gt_group_of=group, gt_difficult=difficult,
                  det_boxes=np.stack(det).astype(np.float32).reshape(-1, 4), det_scores=sc, det_classes=np.asarray(dc, np.int64))
        if labels is not None:
            im['labeled_cls'] = rs.choice(C, size=min(labels, C), replace=False).astype(np.int64)
        images.append(im)
    return images


def pack(images, max_det, M, K=None):
    """0-based images -> numpy det [B,max_det,6] x1,y1,x2,y2,score,class (1-based), count [B] int32, gt_boxes [B,M,4], gt_cls [B,M]
    int64 (1-based, -1 padding), gt_difficult [B,M] uint8, gt_group_of [B,M] uint8, labeled_cls [B,K] int64 (1-based, 0 padding) or
    None when no image carries a list"""
    B = len(images)
    det = np.zeros((B, max_det, 6), np.float32)
    cnt = np.zeros(B, np.int32)
    gtb, gtc = np.zeros((B, M, 4), np.float32), np.full((B, M), -1, np.int64)
    gtd, gtg = np.zeros((B, M), np.uint8), np.zeros((B, M), np.uint8)
    lists = [im.get('labeled_cls') for im in images]
    lab = None
    if any(l is not None for l in lists):
        assert all(l is not None for l in lists)
        K = max([len(l) for l in lists] + [0]) if K is None else K
        lab = np.zeros((B, K), np.int64)
        for i, l in enumerate(lists):
            lab[i, :len(l)] = np.asarray(l, np.int64) + 1
    for i, im in enumerate(images):
        n = len(im['det_scores'])
        b = np.asarray(im['det_boxes'], np.float32).reshape(-1, 4)
        det[i, :n, 0], det[i, :n, 1], det[i, :n, 2], det[i, :n, 3] = b[:, 1], b[:, 0], b[:, 3], b[:, 2]
        det[i, :n, 4] = np.asarray(im['det_scores'], np.float32)
        det[i, :n, 5] = np.asarray(im['det_classes']) + 1
        cnt[i] = n
        m = len(im['gt_classes'])
        gtb[i, :m] = np.asarray(im['gt_boxes'], np.float32).reshape(-1, 4)
        gtc[i, :m] = np.asarray(im['gt_classes'], np.int64) + 1
        gtd[i, :m] = _flags_of(im, 'gt_difficult', m)
        gtg[i, :m] = _flags_of(im, 'gt_group_of', m)
    return det, cnt, gtb, gtc, gtd, gtg, lab


def zero_based(im, group_of=None, difficult=None, labeled=None):
    """an image of tests/_seeded.py::eval_case (1-based classes) in the layout of match_image"""
    out = dict(det_boxes=im['det_boxes'], det_scores=im['det_scores'], det_classes=np.asarray(im['det_classes']) - 1,
               gt_boxes=im['gt_boxes'], gt_classes=np.asarray(im['gt_classes']) - 1)
    if group_of is not None:
        out['gt_group_of'] = np.asarray(group_of, bool)
    if difficult is not None:
        out['gt_difficult'] = np.asarray(difficult, bool)
    if labeled is not None:
        out['labeled_cls'] = np.asarray(labeled, np.int64) - 1
    return out


def fixture_case(g, tag, labels=False, difficult=False):
    """(0-based images of case `tag` of tests/golden/evaluation_openimages.npz with its group-of flags - `difficult`: its difficult
    flags instead, `labels`: with its verified labels -, C)"""
    from _seeded import eval_case
    seed, n_img, C, n_det = [int(v) for v in g[tag + '_meta']]
    images = eval_case(seed, n_img, C, n_det)
    flag = g[tag + ('_difficult' if difficult else '_group_of')].astype(bool)
    lab, lab_n = g[tag + '_labels'], g[tag + '_labels_n']
    out, k, q = [], 0, 0
    for i, im in enumerate(images):
        m = len(im['gt_classes'])
        kw = dict(difficult=flag[k:k + m]) if difficult else dict(group_of=flag[k:k + m])
        out.append(zero_based(im, labeled=lab[q:q + lab_n[i]] if labels else None, **kw))
        k += m
        q += int(lab_n[i])
    assert k == len(flag)
    return out, C
