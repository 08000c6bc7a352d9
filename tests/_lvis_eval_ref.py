"""numpy restatement of the LVIS federated detection evaluation (csrc/lvis_eval.hip) in lvis-api's loop form: `prepare` (the cap of
max_dets[-1] detections an image over all categories, then the images' category sets), `evaluate_img` per (image, category, area
range), `accumulate` per (category, area range), `summarize`.  Written from the rules below; test infrastructure only.

  inputs    per image a dict: det_boxes [n, 4] yxyx, det_scores [n], det_classes [n] 0-based, IN ANY ORDER; gt_boxes [m, 4] yxyx,
            gt_classes [m] 0-based, gt_area [m] (absent: the float32 box area); neg / nel: 0-based categories checked absent /
            not exhaustively annotated (None: every category is judged / none is not-exhaustive).  pos = set(gt_classes).
  valid     the box is not degenerate, the class lies in 0..C-1, the score is not NaN and not < min_score.
  rank      the valid detections of the image in a stable descending sort by score: r = the position.  r >= max_dets[-1]: dropped.
            The cap comes before the filter.
  filter    a detection that survived the cap is dropped iff its class is in neither pos nor neg.
  matching  evaluate_img: the category's boxes ordered not-ignored first (stable), the detections in rank order; a taken box is
            skipped; once a not-ignored match is held the scan stops at the first ignored box; a box whose float32 IoU is not >=
            the best so far (at first: float32 thr_t) is skipped, otherwise it becomes the match, so the LAST box wins on equal
            IoU.  Matched to a not-ignored box: true positive; to an ignored box: ignored; a matched box is taken.
  unmatched ignored iff the detection's own box area is outside [lo_a, hi_a] or its class is in nel; otherwise a false positive.
  flags     [n, A] uint32: bit t true positive, bit 16 + t ignored, bit 31 dropped; rank [n] the image rank (-1: dropped).
  accumulate per (c, a, m): the class's entries (image order, slot order inside an image) with rank < max_dets[m] in a stable
            descending sort by score; tp / fp cumulative over the entries that are not ignored; rc = tp / npig, pr = tp / (fp +
            tp + spacing(1)); pr made non-increasing from the right; q[r] = pr[searchsorted(rc, rec_thr[r], 'left')] or 0 beyond
            the end; AR = rc[-1] or 0 without entries; NaN where npig = 0.  `ap` adds q[0] + q[1] + ... one at a time and divides
            by R (what the device computes); `ap_mean` is np.mean(q).
  summarize the thirteen figures AP, AP50, AP75, APs, APm, APl, APr, APc, APf, AR@k, ARs@k, ARm@k, ARl@k (k = max_dets[-1]): means
            over the cells that are not NaN, -1 without one; APr / APc / APf over the categories of frequency 'r' / 'c' / 'f'.
"""
import numpy as np

F = np.float32
DROPPED = np.uint32(1 << 31)
LVIS_AREAS = ((0.0, 1e5 ** 2), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e5 ** 2))
LVIS_THRESHOLDS = np.linspace(0.5, 0.95, 10)
LVIS_MAX_DETS = (300,)
LVIS_REC_THRS = np.linspace(0.0, 1.0, 101)


def _area(b):
    b = np.asarray(b, F).reshape(-1, 4)
    return (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])


def _iou(d, g):
    """float32 IoU of the boxes d and g (yxyx): inter / ((area_d + area_g) - inter), one rounding per operation"""
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        ih = max(F(0), min(d[2], g[2]) - max(d[0], g[0]))
        iw = max(F(0), min(d[3], g[3]) - max(d[1], g[1]))
        inter = F(ih * iw)
        area_d, area_g = F((d[2] - d[0]) * (d[3] - d[1])), F((g[2] - g[0]) * (g[3] - g[1]))
        return F(inter / F(F(area_d + area_g) - inter))


def _image(im):
    db = np.asarray(im['det_boxes'], F).reshape(-1, 4)
    ds = np.asarray(im['det_scores'], F).reshape(-1)
    dc = np.asarray(im['det_classes']).reshape(-1).astype(np.int64)
    gb = np.asarray(im['gt_boxes'], F).reshape(-1, 4)
    gc = np.asarray(im['gt_classes']).reshape(-1).astype(np.int64)
    ga = np.asarray(im['gt_area'], F).reshape(-1) if im.get('gt_area') is not None else _area(gb)
    return db, ds, dc, gb, gc, ga


def prepare(im, C, cap, min_score=0.0):
    """-> (rank [n] int32: the image rank of a kept detection, -1 dropped; stats: how many the cap / the filter dropped)"""
    db, ds, dc, gb, gc, ga = _image(im)
    valid = np.array([db[i, 0] < db[i, 2] and db[i, 1] < db[i, 3] and 0 <= dc[i] < C and ds[i] == ds[i] and not ds[i] < F(min_score)
                      for i in range(len(ds))], bool)
    idx = np.nonzero(valid)[0]
    idx = idx[np.argsort(-ds[idx], kind='mergesort')]
    rank = np.full(len(ds), -1, np.int32)
    rank[idx[:cap]] = np.arange(min(cap, len(idx)))
    pos = set(int(c) for c in gc if 0 <= c < C)
    judged = None if im.get('neg') is None else pos | set(int(c) for c in im['neg'])
    filtered = 0
    if judged is not None:
        for i in idx[:cap]:
            if int(dc[i]) not in judged:
                rank[i] = -1
                filtered += 1
    return rank, dict(cut=max(0, len(idx) - cap), filtered=filtered)


def evaluate_img(d_boxes, g_boxes, g_area, lo, hi, thresholds, not_exhaustive):
    """one (image, category, area range): detections in rank order.  -> (dt_m [T, D] bool, dt_ig [T, D] bool, boxes that count,
    detections ignored only because the category is not exhaustive)"""
    T, D, G = len(thresholds), len(d_boxes), len(g_boxes)
    gt_ig = np.array([a < F(lo) or a > F(hi) for a in g_area], bool)
    order = np.argsort(gt_ig, kind='mergesort')
    gt_ig = gt_ig[order]
    ious = np.array([[_iou(d, g_boxes[g]) for g in order] for d in d_boxes], F).reshape(D, G)
    dt_m, dt_ig = np.zeros((T, D), bool), np.zeros((T, D), bool)
    for t, thr in enumerate(thresholds):
        gt_m = np.zeros(G, bool)
        for d in range(D):
            best, m = F(thr), -1
            for g in range(G):
                if gt_m[g]:
                    continue
                if m > -1 and not gt_ig[m] and gt_ig[g]:
                    break
                if not ious[d, g] >= best:
                    continue
                best, m = ious[d, g], g
            if m == -1:
                continue
            dt_ig[t, d], dt_m[t, d], gt_m[m] = gt_ig[m], True, True
    d_area = _area(d_boxes) if D else np.zeros(0, F)
    out = np.array([a < F(lo) or a > F(hi) for a in d_area], bool)
    by_nel = int((~dt_m & ~out[None]).any(0).sum()) if not_exhaustive else 0
    dt_ig |= ~dt_m & (out | bool(not_exhaustive))[None]
    return dt_m, dt_ig, int((~gt_ig).sum()), by_nel


def match_image(im, C, thresholds=LVIS_THRESHOLDS, areas=LVIS_AREAS, cap=300, min_score=0.0):
    """-> (flags [n, A] uint32, rank [n] int32, npig [C, A] int64, stats: cut / filtered / nel counts of the image)"""
    db, ds, dc, gb, gc, ga = _image(im)
    T, A = len(thresholds), len(areas)
    rank, stats = prepare(im, C, cap, min_score)
    flags = np.zeros((len(ds), A), np.uint32)
    flags[rank < 0] = DROPPED
    npig = np.zeros((C, A), np.int64)
    nel = set() if im.get('nel') is None else set(int(c) for c in im['nel'])
    stats['nel'] = 0
    cats = sorted(set(int(c) for c in gc if 0 <= c < C) | set(int(c) for c in dc[rank >= 0]))
    for c in cats:
        dets = np.nonzero((rank >= 0) & (dc == c))[0]
        dets = dets[np.argsort(rank[dets], kind='mergesort')]
        g = np.nonzero(gc == c)[0]
        for a, (lo, hi) in enumerate(areas):
            dt_m, dt_ig, count, by_nel = evaluate_img(db[dets], gb[g], ga[g], lo, hi, thresholds, c in nel)
            npig[c, a] += count
            stats['nel'] += by_nel if a == 0 else 0
            for t in range(T):
                flags[dets[dt_m[t] & ~dt_ig[t]], a] |= np.uint32(1 << t)
                flags[dets[dt_ig[t]], a] |= np.uint32(1 << (16 + t))
    return flags, rank, npig, stats


def sorted_entries(scores, classes, C):
    """indices of the entries in the device's order: class, then score descending, equal scores (-0.0 == +0.0) by arrival"""
    scores, classes = np.asarray(scores, F), np.asarray(classes)
    ok = np.nonzero((classes >= 0) & (classes < C) & ~np.isnan(scores))[0]
    ok = ok[np.argsort(-scores[ok], kind='mergesort')]
    return ok[np.argsort(classes[ok], kind='mergesort')]


def accumulate(scores, classes, words, ranks, npig, C, T, max_dets=LVIS_MAX_DETS, rec_thr=LVIS_REC_THRS):
    """LVISEval.accumulate over the kept entries (arrival order).  words [n, A], npig [C, A].
    -> dict(precision [T, R, C, A, Mx], ap, ap_mean, ar: [T, C, A, Mx]); NaN where npig = 0"""
    scores, classes, ranks = np.asarray(scores, F), np.asarray(classes), np.asarray(ranks)
    A = np.asarray(npig).shape[1]
    words = np.asarray(words, np.uint32).reshape(len(scores), A)
    Mx, R = len(max_dets), len(rec_thr)
    rec_thr = np.asarray(rec_thr, np.float64)
    precision = np.full((T, R, C, A, Mx), np.nan)
    ap, ap_mean, ar = (np.full((T, C, A, Mx), np.nan) for _ in range(3))
    for c in range(C):
        of_class = np.nonzero((classes == c) & ~np.isnan(scores))[0]
        for a in range(A):
            num_gt = int(npig[c, a])
            if num_gt == 0:
                continue
            for m, md in enumerate(max_dets):
                use = of_class[ranks[of_class] < md]
                use = use[np.argsort(-scores[use], kind='mergesort')]
                for t in range(T):
                    dt_m = ((words[use, a] >> np.uint32(t)) & 1).astype(bool)
                    dt_ig = ((words[use, a] >> np.uint32(16 + t)) & 1).astype(bool)
                    tp = np.cumsum(dt_m & ~dt_ig).astype(np.float64)
                    fp = np.cumsum(~dt_m & ~dt_ig).astype(np.float64)
                    nd = len(tp)
                    rc = tp / num_gt
                    ar[t, c, a, m] = rc[-1] if nd else 0.0
                    pr = (tp / (fp + tp + np.spacing(1))).tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    q = [0.0] * R
                    for ri, pi in enumerate(np.searchsorted(rc, rec_thr, side='left')):
                        if pi < nd:
                            q[ri] = pr[pi]
                    precision[t, :, c, a, m] = q
                    s = 0.0
                    for v in q:
                        s = s + v
                    ap[t, c, a, m] = s / R
                    ap_mean[t, c, a, m] = np.mean(q)
    return dict(precision=precision, ap=ap, ap_mean=ap_mean, ar=ar)


def summarize(ap, ar, frequency=None, thresholds=LVIS_THRESHOLDS):
    """the thirteen LVIS figures from ap / ar [T, C, 4, Mx] (areas all, small, medium, large; the last max_dets).  frequency: per
    class 'r' / 'c' / 'f' (or None: the three group figures are -1)"""
    thresholds = np.asarray(thresholds, np.float64)

    def one(x, thr=None, a=0, cls=None):
        s = x[:, :, a, -1]
        if cls is not None:
            if not len(cls):
                return -1.0
            s = s[:, cls]
        if thr is not None:
            s = s[np.nonzero(np.abs(thresholds - thr) < 1e-9)[0]]
        s = s[~np.isnan(s)]
        return float(np.mean(s)) if s.size else -1.0
    group = lambda f: [] if frequency is None else [c for c, v in enumerate(frequency) if v == f]
    return np.array([one(ap), one(ap, 0.5), one(ap, 0.75), one(ap, a=1), one(ap, a=2), one(ap, a=3), one(ap, cls=group('r')),
                     one(ap, cls=group('c')), one(ap, cls=group('f')), one(ar), one(ar, a=1), one(ar, a=2), one(ar, a=3)])


def evaluate(images, C, thresholds=LVIS_THRESHOLDS, areas=LVIS_AREAS, max_dets=LVIS_MAX_DETS, rec_thr=LVIS_REC_THRS, min_score=0.0):
    """-> dict(flags: per image [n_i, A], ranks: per image, npig [C, A], scores / classes / words / rank: the kept entries in (image,
    slot) order, nan_scores, stats: cut / filtered / nel totals, and the arrays of `accumulate`)"""
    A = len(areas)
    npig = np.zeros((C, A), np.int64)
    flags, ranks, scores, classes, words, rk, nans = [], [], [], [], [], [], 0
    stats = dict(cut=0, filtered=0, nel=0)
    for im in images:
        f, r, g, st = match_image(im, C, thresholds, areas, max_dets[-1], min_score)
        npig += g
        for k in stats:
            stats[k] += st[k]
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
               words=cat(words, np.uint32, (0, A)), rank=cat(rk, np.int32, 0), nan_scores=nans, stats=stats)
    out.update(accumulate(out['scores'], out['classes'], out['words'], out['rank'], npig, C, len(thresholds), max_dets, rec_thr))
    return out


def pack(images, max_det, M, Kn=None, Ke=None, with_area=None):
    """images -> det [B, max_det, 6] x1, y1, x2, y2, score, 1-based class; count [B] int32; gt_boxes [B, M, 4]; gt_cls [B, M] int64
    1-based (-1 padding); gt_area [B, M] float32 or None (None unless an image has 'gt_area'); neg_cls [B, Kn] / nel_cls [B, Ke]
    int64 1-based (-1 padding), None when every image's list is None.  Kn / Ke default to the longest list (0 is allowed)."""
    B = len(images)
    if with_area is None:
        with_area = any(im.get('gt_area') is not None for im in images)
    det, cnt = np.zeros((B, max_det, 6), F), np.zeros(B, np.int32)
    gtb, gtc, area = np.zeros((B, M, 4), F), np.full((B, M), -1, np.int64), np.zeros((B, M), F)
    for i, im in enumerate(images):
        db, ds, dc, gb, gc, ga = _image(im)
        n, m = len(ds), len(gc)
        det[i, :n, 0], det[i, :n, 1], det[i, :n, 2], det[i, :n, 3] = db[:, 1], db[:, 0], db[:, 3], db[:, 2]
        det[i, :n, 4], det[i, :n, 5] = ds, dc + 1
        cnt[i] = n
        gtb[i, :m], gtc[i, :m], area[i, :m] = gb, gc + 1, ga

    def lists(key, K):
        if all(im.get(key) is None for im in images):
            return None
        rows = [list(im.get(key) or ()) for im in images]
        K = max(len(r) for r in rows) if K is None else K
        out = np.full((B, K), -1, np.int64)
        for i, r in enumerate(rows):
            out[i, :len(r)] = np.asarray(r, np.int64) + 1
        return out
    return det, cnt, gtb, gtc, (area if with_area else None), lists('neg', Kn), lists('nel', Ke)


def random_images(seed, n_img, C, M, n_det, n_neg=2, n_nel=1, grid=8.0, size=160.0, scores_levels=0, gt_classes=None):
    """Images whose boxes lie on a coarse integer grid (equal IoUs, IoUs exactly on a threshold, areas exactly 32^2, duplicate boxes
    all occur); the detections are jittered copies of ground truth plus strays with classes from -1 .. C, IN A SHUFFLED ORDER; neg:
    n_neg random categories (n_neg = None: no list, n_neg >= C: all); nel: n_nel of the judged categories that have detections
    in the image (n_nel = None: no list).  gt_classes: the most distinct classes the boxes of an image have (default: any).  scores_levels > 0: scores are
    multiples of 1 / scores_levels (ties)."""
    rs = np.random.RandomState(seed)
    sides = [8, 16, 32, 32, 64, 96, 128]
    out = []
    for _ in range(n_img):
        m = M if rs.uniform() < 0.5 or M <= 1 else int(rs.randint(0, M + 1))
        y0, x0 = rs.randint(0, int(size / grid), m) * grid, rs.randint(0, int(size / grid), m) * grid
        gb = np.stack([y0, x0, y0 + rs.choice(sides, m), x0 + rs.choice(sides, m)], 1).astype(F).reshape(-1, 4)
        pool = rs.permutation(C)[:gt_classes] if gt_classes else np.arange(C)
        gc = pool[rs.randint(0, len(pool), m)]
        n = int(rs.randint(0, n_det + 1)) if rs.uniform() < 0.3 and out else n_det       # the first image has all n_det rows
        db, dc = np.zeros((n, 4), F), rs.randint(-1, C + 1, n)
        for k in range(n):
            if m and rs.uniform() < 0.75:
                j = rs.randint(0, m)
                db[k] = gb[j] + rs.choice([0, 0, grid, -grid, grid / 2], 4)
                dc[k] = gc[j] if rs.uniform() < 0.8 else dc[k]
            else:
                yy, xx = rs.randint(0, int(size / grid), 2) * grid
                db[k] = (yy, xx, yy + rs.choice([8, 32, 64]), xx + rs.choice([8, 32, 64]))
        ds = (rs.randint(0, scores_levels + 1, n) / F(scores_levels)).astype(F) if scores_levels else rs.uniform(0, 1, n).astype(F)
        neg = None if n_neg is None else (list(range(C)) if n_neg >= C else sorted(rs.permutation(C)[:n_neg].tolist()))
        judged = set(range(C)) if neg is None else set(gc.tolist()) | set(neg)
        seen = sorted(judged & set(int(c) for c in dc)) or sorted(judged)     # judged categories that have detections, if any
        nel = None if n_nel is None else sorted(rs.permutation(seen)[:n_nel].tolist())
        out.append(dict(gt_boxes=gb, gt_classes=gc, det_boxes=db, det_scores=ds, det_classes=dc, neg=neg, nel=nel))
    return out
