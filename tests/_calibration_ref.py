"""numpy restatement of the detection calibration unit (csrc/calibration_eval.hip), in float64; float32 only where the device uses
it: the IoU (oracle.evaluation.iou_matrix) and the width-bin product p * K.  Test infrastructure only.

  match_image     the matching of tests/_eval_scale_ref.py (its flag words are asserted equal) and per detection the IoU with its
                  candidate: the box of its class with the largest IoU, the lowest index on ties; 0 without a box or when dropped
  accumulate      the kept entries (not dropped, score >= score_threshold) in arrival order
  tables          both sorts, both binning schemes, the per-bin sums (math.fsum: correctly rounded) and brier / nll / out_of_range
  metrics         D-ECE, MCE, ACE, classwise-ECE, LaECE, Brier, NLL from a table dict, the operations in the order of
                  effdet/evaluation/calibration_evaluator.py::calibration_metrics
  newton_fit      the damped Newton state machine of the fit, from (1, 0)
  apply_scores    p' = float32(sigmoid(a logit(p~) + b))
"""
import math

import numpy as np

import _eval_scale_ref as S
from oracle.evaluation import iou_matrix

INVALID = S.INVALID
LO, HI = 2.0 ** -24, 1.0 - 2.0 ** -24
SLACK, TOL, MIN_STEP = 1.0 + 2.0 ** -40, 2.0 ** -40, 2.0 ** -60


# ---- matching ------------------------------------------------------------------------------------------------------------------------
def match_image(im, num_classes, thresholds):
    """-> (flag words [n] uint32 as _eval_scale_ref.match_image, candidate IoU [n] float32, correct [T, C])"""
    flags, correct = S.match_image(im, num_classes, thresholds)
    det_boxes = np.asarray(im['det_boxes'], np.float32).reshape(-1, 4)
    det_classes = np.asarray(im['det_classes']).reshape(-1)
    gt_boxes = np.asarray(im['gt_boxes'], np.float32).reshape(-1, 4)
    gt_classes = np.asarray(im['gt_classes']).reshape(-1)
    iou = np.zeros(len(det_classes), np.float32)
    for i in range(len(det_classes)):
        if flags[i] & INVALID:
            continue
        g = np.nonzero(gt_classes == det_classes[i])[0]
        if g.size:
            row = iou_matrix(det_boxes[i:i + 1], gt_boxes[g])[0]
            iou[i] = row[int(np.argmax(row))]                                  # the first maximum
    return flags, iou, correct


def accumulate(images, num_classes, thresholds, score_threshold=0.0):
    """-> dict(scores float32, classes int64, flags uint32, iou float32: the kept entries in (image, slot) order; per_image: the
    (flags, iou) of every slot; gt_count, gt_imgs [C], correct [T, C], nan_scores)"""
    T = len(thresholds)
    sc, cl, fl, io, per = [], [], [], [], []
    gt_count, gt_imgs = np.zeros(num_classes, np.int64), np.zeros(num_classes, np.int64)
    correct = np.zeros((T, num_classes), np.int64)
    nans = 0
    thr = np.float32(score_threshold)
    for im in images:
        f, u, cor = match_image(im, num_classes, thresholds)
        per.append((f, u))
        correct += cor
        gc = np.asarray(im['gt_classes']).reshape(-1)
        dif = np.asarray(im.get('gt_difficult', np.zeros(len(gc))), bool).reshape(-1)
        for c in range(num_classes):
            gt_count[c] += int(np.sum((gc == c) & ~dif))
            gt_imgs[c] += 1 if np.any(gc == c) else 0
        s = np.asarray(im['det_scores'], np.float32).reshape(-1)
        nans += int(np.isnan(s).sum())
        with np.errstate(invalid='ignore'):
            keep = ((f & INVALID) == 0) & (s >= thr)
        sc.append(s[keep] + np.float32(0)), cl.append(np.asarray(im['det_classes'], np.int64).reshape(-1)[keep])
        fl.append(f[keep]), io.append(u[keep])
    cat = lambda v, dt: np.concatenate(v).astype(dt) if v else np.zeros(0, dt)
    return dict(scores=cat(sc, np.float32), classes=cat(cl, np.int64), flags=cat(fl, np.uint32), iou=cat(io, np.float32),
                per_image=per, gt_count=gt_count, gt_imgs=gt_imgs, correct=correct, nan_scores=nans)


# ---- tables --------------------------------------------------------------------------------------------------------------------------
def width_bin(p, K):
    """k = min(K - 1, max(0, (int)(p * (float)K))), the product in float32"""
    q = np.asarray(p, np.float32) * np.float32(K)
    with np.errstate(invalid='ignore'):
        return np.where(q >= np.float32(K), K - 1, np.where(q > 0, np.minimum(q, np.float32(K)).astype(np.int64), 0)).astype(np.int64)


def sorted_scopes(scores, classes, num_classes):
    """-> (order of the class sort, order of the pooled sort): indices into the entries.  Class, then score descending, equal
    scores by arrival; the pooled order re-sorts the class order by score alone (equal scores by class, then arrival)."""
    scores = np.asarray(scores, np.float32)
    ok = np.nonzero((classes >= 0) & (classes < num_classes) & ~np.isnan(scores))[0]
    o = ok[np.argsort(-scores[ok], kind='stable')]
    o = o[np.argsort(classes[o], kind='stable')]
    return o, o[np.argsort(-scores[o], kind='stable')]


def tables(scores, classes, flags, iou, num_classes, T, K):
    """the result block of the device as arrays (the layout of parse_calibration_result, without the head and the counters)"""
    scores, iou = np.asarray(scores, np.float32), np.asarray(iou, np.float32)
    classes, flags = np.asarray(classes, np.int64), np.asarray(flags, np.uint32)
    C, S_ = num_classes, num_classes + 1
    order, pooled = sorted_scopes(scores, classes, C)
    n = np.zeros((T, S_, 2, K), np.int64)
    tp = np.zeros((T, S_, 2, K), np.int64)
    sum_p, sum_iou = np.zeros((T, S_, 2, K)), np.zeros((T, S_, 2, K))
    brier, nll = np.zeros((T, S_)), np.zeros((T, S_))
    oor, entries = np.zeros((T, S_), np.int64), np.zeros((T, S_), np.int64)
    for s in range(S_):
        idx = pooled if s == C else order[classes[order] == s]
        m = len(idx)
        p32, u32, f = scores[idx], iou[idx], flags[idx]
        p, u = p32.astype(np.float64), u32.astype(np.float64)
        wbin = width_bin(p32, K)
        mbin = np.zeros(m, np.int64)
        for k in range(K):
            mbin[(k * m) // K:((k + 1) * m) // K] = k
        for t in range(T):
            live = ((f >> np.uint32(16 + t)) & 1) == 0
            pos = (((f >> np.uint32(t)) & 1) == 1) & live
            entries[t, s] = m
            for z, b in enumerate((wbin, mbin)):
                for k in range(K):
                    sel = live & (b == k)
                    n[t, s, z, k] = int(sel.sum())
                    tp[t, s, z, k] = int((sel & pos).sum())
                    sum_p[t, s, z, k] = math.fsum(p[sel])
                    sum_iou[t, s, z, k] = math.fsum(u[sel & pos])
            y = pos[live].astype(np.float64)
            pl = p[live]
            pc = np.minimum(np.maximum(pl, LO), HI)
            brier[t, s] = math.fsum((pl - y) * (pl - y))
            nll[t, s] = math.fsum(-np.log(np.where(y > 0, pc, 1.0 - pc)))
            oor[t, s] = int((~((p32[live] >= 0) & (p32[live] <= 1))).sum())
    return dict(bins=dict(n=n, tp=tp, sum_p=sum_p, sum_iou=sum_iou), brier=brier, nll=nll, out_of_range=oor, entries=entries)


# ---- metrics ---------------------------------------------------------------------------------------------------------------------------
def gap_sum(n, a, b):
    total = int(np.sum(n))
    if total == 0:
        return float('nan'), float('nan')
    ece, mce = 0.0, 0.0
    for k in range(len(n)):
        if n[k] == 0:
            continue
        nk = float(n[k])
        gap = abs(float(a[k]) / nk - float(b[k]) / nk)
        ece = ece + (nk / float(total)) * gap
        mce = max(mce, gap)
    return ece, mce


def metrics(r, t):
    b = r['bins']
    C = b['n'].shape[1] - 1
    d_ece, mce = gap_sum(b['n'][t, C, 0], b['sum_p'][t, C, 0], b['tp'][t, C, 0])
    ace, _ = gap_sum(b['n'][t, C, 1], b['sum_p'][t, C, 1], b['tp'][t, C, 1])
    cw, la = [], []
    for c in range(C):
        if int(b['n'][t, c, 0].sum()) == 0:
            continue
        cw.append(gap_sum(b['n'][t, c, 0], b['sum_p'][t, c, 0], b['tp'][t, c, 0])[0])
        la.append(gap_sum(b['n'][t, c, 0], b['sum_p'][t, c, 0], b['sum_iou'][t, c, 0])[0])
    n = int(b['n'][t, C, 0].sum())
    mean = lambda v: float(np.sum(np.asarray(v, np.float64)) / len(v)) if v else float('nan')
    return {'D-ECE': d_ece, 'MCE': mce, 'ACE': ace, 'classwise-ECE': mean(cw), 'LaECE': mean(la),
            'Brier': float(r['brier'][t, C]) / n if n else float('nan'), 'NLL': float(r['nll'][t, C]) / n if n else float('nan')}


# ---- the fit ---------------------------------------------------------------------------------------------------------------------------
def logit(p):
    c = np.minimum(np.maximum(np.asarray(p, np.float64), LO), HI)
    return np.log(c / (1.0 - c))


def sigmoid(z):
    z = np.asarray(z, np.float64)
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def fit_data(scores, flags, iou, t, target):
    """(x, y) of the entries that take part in the fit at threshold index t"""
    scores, flags = np.asarray(scores, np.float32), np.asarray(flags, np.uint32)
    use = ((flags & INVALID) == 0) & (((flags >> np.uint32(16 + t)) & 1) == 0) & ~np.isnan(scores)
    tp = ((flags[use] >> np.uint32(t)) & 1) == 1
    y = np.where(tp, np.asarray(iou, np.float32)[use].astype(np.float64) if target == 'iou' else 1.0, 0.0)
    return logit(scores[use]), y


def _pairwise(v):
    v = np.asarray(v, np.float64)
    while len(v) > 1:
        if len(v) & 1:
            v = np.concatenate([v, [0.0]])
        v = v[0::2] + v[1::2]
    return float(v[0]) if len(v) else 0.0


def _sequential(v):
    s = 0.0
    for x in np.asarray(v, np.float64).tolist():
        s = s + x
    return s


SUMS = dict(sequential=_sequential, pairwise=_pairwise, fsum=lambda v: math.fsum(np.asarray(v, np.float64).tolist()))


def fit_sums(x, y, a, b, add):
    z = a * x + b
    e = np.exp(-np.abs(z))
    sg = np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    d, w = sg - y, sg * (1.0 - sg)
    return (add((np.log1p(e) + np.maximum(z, 0.0)) - y * z), add(d * x), add(d), add((w * x) * x), add(w * x), add(w))


def newton_fit(x, y, method='platt', max_iter=32, summation='pairwise'):
    """the state machine of ca_fit_update_kernel -> dict(a, b, iterations, halvings, converged, nll_before, nll_after, gradient)"""
    add = SUMS[summation]
    a, b, nll = 1.0, 0.0, 0.0
    ta, tb, lam, da, db = 1.0, 0.0, 1.0, 0.0, 0.0
    nll0, iters, halv, conv, frozen, have = 0.0, 0, 0, False, False, False
    grad = (float('nan'), float('nan'))
    for _ in range(max_iter):
        if frozen:
            break
        L, ga, gb, haa, hab, hbb = fit_sums(x, y, ta, tb, add)
        iters += 1
        if not have:
            if not math.isfinite(L):
                frozen = True
                continue
            nll0 = L
        elif not (math.isfinite(L) and L <= nll * SLACK):
            lam = lam * 0.5
            halv += 1
            ta, tb = a + lam * da, b + lam * db
            if lam < MIN_STEP:
                frozen = True
            continue
        a, b, nll, have, grad = ta, tb, L, True, (ga, gb)
        with np.errstate(all='ignore'):
            if method == 'temperature':
                ok = haa > 0.0
                da, db = (-(ga / haa) if haa != 0 else float('nan')), 0.0
            else:
                det = haa * hbb - hab * hab
                ok = det > 0.0 and haa > 0.0
                da = -((hbb * ga - hab * gb) / det) if det != 0 else float('nan')
                db = -((haa * gb - hab * ga) / det) if det != 0 else float('nan')
        if not ok or not math.isfinite(da) or not math.isfinite(db):
            frozen = True
            continue
        if max(abs(da), abs(db)) <= TOL * max(1.0, abs(a), abs(b)):
            conv, frozen = True, True
            continue
        lam = 1.0
        ta, tb = a + da, b + db
    return dict(a=a, b=b, iterations=iters, halvings=halv, converged=conv, nll_before=nll0, nll_after=nll, gradient=grad)


def apply_scores(p, a, b):
    """float32 scores -> float32(sigmoid(a logit(p~) + b))"""
    return sigmoid(a * logit(np.asarray(p, np.float32)) + b).astype(np.float32)


def apply_det(det, count, a, b):
    out = np.array(det, np.float32, copy=True)
    for i in range(out.shape[0]):
        n = min(int(count[i]), out.shape[1])
        out[i, :n, 4] = apply_scores(out[i, :n, 4], a, b)
    return out


def bernoulli_case(seed, n, a0, b0):
    """float32 scores in (0, 1) and Bernoulli labels whose true calibration map is (a0, b0): flag words (bit 0 = tp) and IoU"""
    rs = np.random.RandomState(seed)
    scores = rs.uniform(0.02, 0.98, n).astype(np.float32)
    q = sigmoid(a0 * logit(scores) + b0)
    tp = rs.uniform(size=n) < q
    iou = np.where(tp, rs.uniform(0.5, 1.0, n), rs.uniform(0.0, 0.5, n)).astype(np.float32)
    return scores, tp.astype(np.uint32), iou


FIT_CASES = [(300, 1.5, -0.5), (4097, 0.6, 0.3), (70000, 2.5, -1.0), (4097, 0.05, 2.0), (2049, 8.0, 0.0)]
