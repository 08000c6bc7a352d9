"""numpy restatement of the COCO-protocol detection evaluation (csrc/coco_eval.hip): COCOeval.evaluateImg / accumulate /
summarize of pycocotools for iouType 'bbox', with float32 IoU and float32 IoU thresholds.  Test infrastructure only.

Definitions (the unit's header comment states the same):
  inputs    per image: detections (boxes yxyx, scores, 0-based classes) in descending score order; ground truth boxes yxyx,
            0-based classes, `gt_crowd` flags and `gt_area` (absent: the float32 box area (y2 - y1) * (x2 - x1)).
  dropped   a detection with a degenerate box, a class outside 0..C-1, a NaN score, a score < min_score, or whose 0-based rank
            among the kept detections of its class in the image is >= max_dets[-1] (computeIoU truncates before matching).
  IoU       float32, inter / ((area_d + area_g) - inter); against a crowd box inter / area_d (maskApi bbIou with iscrowd).
  ignore    box g is ignored at area range a iff it is crowd, or area_g < lo_a, or area_g > hi_a (evaluateImg: g['_ignore']).
  matching  per (t, a), detections in order: the ground truth of the class is ordered not-ignored first (a stable sort); a box
            that is taken at (t, a) and not crowd is skipped; once a not-ignored match is held the scan stops at the first ignored
            box; a box whose IoU is below the best so far (at first: thr_t) is skipped, otherwise it becomes the match - so the
            LAST box wins on equal IoU.  pycocotools compares with min(thr, 1 - 1e-10) in float64; here the comparison is
            IoU >= thr_t in float32.  Matched to a not-ignored box: true positive.  Matched to an ignored box: the detection is
            ignored.  Unmatched: ignored iff its own box area is outside [lo_a, hi_a], else a false positive.
  flags     [n, A] uint32: bit t true positive, bit 16 + t ignored, bit 31 dropped; rank [n] (-1: dropped).
  npig      [C, A] boxes of class c not ignored at a.
  accumulate per (t, c, a, m): the class's entries in (score descending, arrival order) with rank < max_dets[m]; tps / fps exclude
            the ignored ones; rc = tp / npig, pr = tp / (fp + tp + spacing(1)); pr made non-increasing from the right;
            q[r] = pr[searchsorted(rc, rec_thr[r], 'left')] or 0 beyond the end; recall = rc[-1] or 0 without entries;
            precision and recall stay NaN (pycocotools: -1) where npig = 0.
  AP        mean of q over r: `ap` adds q[0] + q[1] + ... one at a time and divides by R (what the device computes, bit for bit);
            `ap_mean` is np.mean(q) (pairwise), what pycocotools' summarize would give for one cell.
"""
import numpy as np

DROPPED = np.uint32(1 << 31)
COCO_AREAS = ((0.0, 1e5 ** 2), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e5 ** 2))
COCO_THRESHOLDS = np.linspace(0.5, 0.95, 10)
COCO_MAX_DETS = (1, 10, 100)
COCO_REC_THRS = np.linspace(0.0, 1.0, 101)
F = np.float32


def box_area(b):
    b = np.asarray(b, F).reshape(-1, 4)
    return (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])


def iou_row(d, g, crowd):
    """float32 IoU of one detection box d (yxyx) with boxes g [m, 4]; crowd [m] bool: intersection over the detection's area"""
    d, g = np.asarray(d, F), np.asarray(g, F).reshape(-1, 4)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        area_d = (d[2] - d[0]) * (d[3] - d[1])
        ih = np.maximum(F(0), np.minimum(d[2], g[:, 2]) - np.maximum(d[0], g[:, 0]))
        iw = np.maximum(F(0), np.minimum(d[3], g[:, 3]) - np.maximum(d[1], g[:, 1]))
        inter = ih * iw
        area_g = (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1])
        return np.where(crowd, inter / area_d, inter / (area_d + area_g - inter)).astype(F)


def _fields(im):
    gc = np.asarray(im['gt_classes']).reshape(-1)
    gb = np.asarray(im['gt_boxes'], F).reshape(-1, 4)
    crowd = np.asarray(im.get('gt_crowd', np.zeros(len(gc))), bool).reshape(-1)
    area = np.asarray(im['gt_area'], F).reshape(-1) if im.get('gt_area') is not None else box_area(gb)
    return (np.asarray(im['det_boxes'], F).reshape(-1, 4), np.asarray(im['det_scores'], F).reshape(-1),
            np.asarray(im['det_classes']).reshape(-1), gb, gc, crowd, area)


def kept_ranks(im, C, max_rank, min_score=0.0):
    """[n] the 0-based rank of a detection among the kept ones of its class, -1 for a dropped one"""
    db, ds, dc, *_ = _fields(im)
    ranks = np.full(len(ds), -1, np.int32)
    seen = {}
    for i in range(len(ds)):
        ok = db[i, 0] < db[i, 2] and db[i, 1] < db[i, 3] and 0 <= dc[i] < C and ds[i] == ds[i] and not ds[i] < F(min_score)
        if ok and seen.get(int(dc[i]), 0) < max_rank:
            ranks[i] = seen.get(int(dc[i]), 0)
            seen[int(dc[i])] = ranks[i] + 1
    return ranks


def gt_ignore(crowd, area, areas):
    """[A, m] bool"""
    return np.stack([crowd | (area < F(lo)) | (area > F(hi)) for lo, hi in areas]) if len(areas) else np.zeros((0, len(crowd)), bool)


def match_image(im, C, thresholds=COCO_THRESHOLDS, areas=COCO_AREAS, max_rank=100, min_score=0.0, literal=False):
    """-> (flags [n, A] uint32, ranks [n] int32, npig [C, A] int64).  literal: the inner scan over the ground truth as the loop
    of COCOeval.evaluateImg; otherwise the same choice by array operations (tests/test_coco_eval_host.py holds the two equal)."""
    db, ds, dc, gb, gc, crowd, area = _fields(im)
    T, A, n = len(thresholds), len(areas), len(ds)
    thr = [F(t) for t in thresholds]
    ranks = kept_ranks(im, C, max_rank, min_score)
    flags = np.zeros((n, A), np.uint32)
    flags[ranks < 0] = DROPPED
    ig_all = gt_ignore(crowd, area, areas)
    npig = np.zeros((C, A), np.int64)
    for c in range(C):
        npig[c] = (~ig_all[:, gc == c]).sum(1)
    d_area = box_area(db)
    for c in range(C):
        dets = np.nonzero((ranks >= 0) & (dc == c))[0]
        g = np.nonzero(gc == c)[0]
        if dets.size == 0:
            continue
        rows = [iou_row(db[i], gb[g], crowd[g]) for i in dets]
        for a, (lo, hi) in enumerate(areas):
            gt_ig = ig_all[a, g]
            order = np.argsort(gt_ig, kind='mergesort')                       # not ignored first, original order inside
            ig_s, crowd_s = gt_ig[order], crowd[g][order]
            for t in range(T):
                taken = np.zeros(g.size, bool)                                # gtm > 0, in the sorted order
                for k, i in enumerate(dets):
                    row = rows[k][order]
                    if literal:
                        best, m = thr[t], -1
                        for gi in range(g.size):
                            if taken[gi] and not crowd_s[gi]:
                                continue
                            if m > -1 and not ig_s[m] and ig_s[gi]:
                                break
                            if not row[gi] >= best:
                                continue
                            best, m = row[gi], gi
                    else:
                        m = -1
                        for group in (~ig_s, ig_s):
                            cand = np.nonzero(group & ~(taken & ~crowd_s) & (row >= thr[t]))[0]
                            if cand.size:
                                top = row[cand].max()
                                m = int(cand[row[cand] == top][-1])           # the last index on equal IoU
                                break
                    if m >= 0:
                        taken[m] = True
                        flags[i, a] |= np.uint32(1 << (16 + t)) if ig_s[m] else np.uint32(1 << t)
                    elif d_area[i] < F(lo) or d_area[i] > F(hi):
                        flags[i, a] |= np.uint32(1 << (16 + t))
    return flags, ranks, npig


def sorted_entries(scores, classes, C):
    """indices of the entries in the device's order: class, then score descending, equal scores (-0.0 == +0.0) by arrival"""
    scores, classes = np.asarray(scores, F), np.asarray(classes)
    ok = np.nonzero((classes >= 0) & (classes < C) & ~np.isnan(scores))[0]
    ok = ok[np.argsort(-scores[ok], kind='stable')]
    return ok[np.argsort(classes[ok], kind='stable')]


def accumulate(scores, classes, words, ranks, npig, C, T, max_dets=COCO_MAX_DETS, rec_thr=COCO_REC_THRS):
    """COCOeval.accumulate over the kept entries (arrival order).  words [n, A], npig [C, A].
    -> dict(precision [T, R, C, A, Mx], ap, ap_mean, ar: [T, C, A, Mx]); NaN where npig = 0"""
    scores, classes, ranks = np.asarray(scores, F), np.asarray(classes), np.asarray(ranks)
    words = np.asarray(words, np.uint32).reshape(len(scores), -1)
    A, Mx, R = words.shape[1] if len(scores) else np.asarray(npig).shape[1], len(max_dets), len(rec_thr)
    rec_thr = np.asarray(rec_thr, np.float64)
    precision = np.full((T, R, C, A, Mx), np.nan)
    ap, ap_mean, ar = (np.full((T, C, A, Mx), np.nan) for _ in range(3))
    order = sorted_entries(scores, classes, C)
    for c in range(C):
        seg = order[classes[order] == c]
        for a in range(A):
            if npig[c, a] == 0:
                continue
            for m, md in enumerate(max_dets):
                use = seg[ranks[seg] < md]
                w = words[use, a]
                for t in range(T):
                    ig = ((w >> np.uint32(16 + t)) & 1).astype(bool)
                    tpb = ((w >> np.uint32(t)) & 1).astype(bool)
                    tp = np.cumsum(tpb & ~ig).astype(np.float64)
                    fp = np.cumsum(~tpb & ~ig).astype(np.float64)
                    nd = len(tp)
                    rc = tp / npig[c, a]
                    pr = tp / (fp + tp + np.spacing(1))
                    q = np.zeros(R)
                    pr = pr.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    inds = np.searchsorted(rc, rec_thr, side='left')
                    for ri, pi in enumerate(inds):
                        if pi < nd:
                            q[ri] = pr[pi]
                    precision[t, :, c, a, m] = q
                    s = 0.0
                    for v in q:
                        s = s + v
                    ap[t, c, a, m] = s / R
                    ap_mean[t, c, a, m] = np.mean(q)
                    ar[t, c, a, m] = rc[-1] if nd else 0.0
    return dict(precision=precision, ap=ap, ap_mean=ap_mean, ar=ar)


def summarize(ap, ar, thresholds=COCO_THRESHOLDS, max_dets=COCO_MAX_DETS):
    """COCOeval.summarize: the 12 figures of `stats` from ap / ar [T, C, 4, Mx] (areas all, small, medium, large); NaN = -1 there"""
    thresholds = np.asarray(thresholds, np.float64)

    def one(x, thr, a, m):
        s = x[:, :, a, m]
        if thr is not None:
            s = s[np.nonzero(np.abs(thresholds - thr) < 1e-9)[0]]
        s = s[~np.isnan(s)]
        return float(np.mean(s)) if s.size else -1.0
    last = len(max_dets) - 1
    return np.array([one(ap, None, 0, last), one(ap, 0.5, 0, last), one(ap, 0.75, 0, last), one(ap, None, 1, last),
                     one(ap, None, 2, last), one(ap, None, 3, last), one(ar, None, 0, 0), one(ar, None, 0, min(1, last)),
                     one(ar, None, 0, last), one(ar, None, 1, last), one(ar, None, 2, last), one(ar, None, 3, last)])


def evaluate(images, C, thresholds=COCO_THRESHOLDS, areas=COCO_AREAS, max_dets=COCO_MAX_DETS, rec_thr=COCO_REC_THRS, min_score=0.0):
    """-> dict(flags: per image [n_i, A], ranks: per image, npig [C, A], scores / classes / words / rank: the kept entries in (image,
    slot) order, nan_scores, and the arrays of `accumulate`)"""
    A = len(areas)
    npig = np.zeros((C, A), np.int64)
    flags, ranks, scores, classes, words, rk, nans = [], [], [], [], [], [], 0
    for im in images:
        f, r, g = match_image(im, C, thresholds, areas, max_dets[-1], min_score)
        npig += g
        flags.append(f)
        ranks.append(r)
        keep = r >= 0
        ds = np.asarray(im['det_scores'], F).reshape(-1)
        nans += int(np.isnan(ds).sum())
        scores.append(ds[keep])
        classes.append(np.asarray(im['det_classes'], np.int64).reshape(-1)[keep])
        words.append(f[keep])
        rk.append(r[keep])
    cat = lambda v, dt, shape: np.concatenate(v) if v else np.zeros(shape, dt)
    out = dict(flags=flags, ranks=ranks, npig=npig, scores=cat(scores, F, 0), classes=cat(classes, np.int64, 0),
               words=cat(words, np.uint32, (0, A)), rank=cat(rk, np.int32, 0), nan_scores=nans)
    out.update(accumulate(out['scores'], out['classes'], out['words'], out['rank'], npig, C, len(thresholds), max_dets, rec_thr))
    return out


def pack(images, max_det, M, with_area=None):
    """images -> det [B, max_det, 6] x1, y1, x2, y2, score, 1-based class; count [B] int32; gt_boxes [B, M, 4]; gt_cls [B, M] int64
    1-based (-1 padding); gt_crowd [B, M] uint8; gt_area [B, M] float32 or None (None unless an image has 'gt_area')"""
    B = len(images)
    if with_area is None:
        with_area = any(im.get('gt_area') is not None for im in images)
    det, cnt = np.zeros((B, max_det, 6), F), np.zeros(B, np.int32)
    gtb, gtc = np.zeros((B, M, 4), F), np.full((B, M), -1, np.int64)
    crowd, area = np.zeros((B, M), np.uint8), np.zeros((B, M), F)
    for i, im in enumerate(images):
        db, ds, dc, gb, gc, cr, ar = _fields(im)
        n, m = len(ds), len(gc)
        det[i, :n, 0], det[i, :n, 1], det[i, :n, 2], det[i, :n, 3] = db[:, 1], db[:, 0], db[:, 3], db[:, 2]
        det[i, :n, 4], det[i, :n, 5] = ds, dc + 1
        cnt[i] = n
        gtb[i, :m], gtc[i, :m], crowd[i, :m], area[i, :m] = gb, gc + 1, cr, ar
    return det, cnt, gtb, gtc, crowd, (area if with_area else None)


def random_images(seed, n_img, C, M, n_det, crowd_frac=0.15, grid=8.0, size=160.0, scores_levels=0):
    """Images whose boxes lie on a coarse integer grid, so that equal IoUs, IoUs exactly on a threshold, boxes of area exactly 32^2
    and duplicate boxes all occur; detections are jittered copies of ground truth plus strays, in descending score order.
    scores_levels > 0: scores are multiples of 1 / scores_levels (ties inside and across images)."""
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(n_img):
        m = int(rs.randint(0, M + 1)) if M > 1 else M
        m = M if rs.uniform() < 0.5 else m
        y0 = rs.randint(0, int(size / grid), m) * grid
        x0 = rs.randint(0, int(size / grid), m) * grid
        h = rs.choice([8, 16, 32, 32, 64, 96, 128], m).astype(float)
        w = rs.choice([8, 16, 32, 32, 64, 96, 128], m).astype(float)
        gb = np.stack([y0, x0, y0 + h, x0 + w], 1).astype(F).reshape(-1, 4)
        gc = rs.randint(0, C, m)
        cr = rs.uniform(size=m) < crowd_frac
        n = int(rs.randint(0, n_det + 1)) if rs.uniform() < 0.3 else n_det
        db = np.zeros((n, 4), F)
        dc = rs.randint(-1, C + 1, n)
        for k in range(n):
            if m and rs.uniform() < 0.75:
                j = rs.randint(0, m)
                jit = rs.choice([0, 0, grid, -grid, grid / 2], 4)
                db[k] = gb[j] + jit
                dc[k] = gc[j] if rs.uniform() < 0.9 else dc[k]
            else:
                yy, xx = rs.randint(0, int(size / grid), 2) * grid
                db[k] = (yy, xx, yy + rs.choice([8, 32, 64]), xx + rs.choice([8, 32, 64]))
        if scores_levels:
            ds = (rs.randint(0, scores_levels + 1, n) / F(scores_levels)).astype(F)
        else:
            ds = rs.uniform(0, 1, n).astype(F)
        ds = -np.sort(-ds)
        out.append(dict(gt_boxes=gb, gt_classes=gc, gt_crowd=cr, det_boxes=db, det_scores=ds, det_classes=dc))
    return out
