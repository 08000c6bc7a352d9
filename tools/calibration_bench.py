#!/usr/bin/env python
"""Time of the detection calibration unit (effdet.evaluation.CalibrationEvaluator and calibration.DetectionCalibrator,
csrc/calibration_eval.hip) beside the torch composition of the same figures:

  add_batch   one batch of 64 images x 100 detections, 80 classes, 10 IoU thresholds (matching with the candidate IoU + append),
              beside DatasetDetectionEvaluator.add_batch on the same batch in the same process;
  enqueue()   both sorts + the tables over n accumulated detections, C = 80, T = 10, K = 15; nothing is read back.  Beside it the
              torch composition of ONE threshold's pooled and per-class equal-width tables: torch.sort by score, the stable sort by
              class, torch.bucketize, and index_add_ of n, tp, sum_p and sum_iou in float64 (it leaves out the equal-mass scheme,
              nine thresholds and brier / nll);
  fit         32 enqueued Newton iterations over the same entries, beside a torch Newton loop of the same formulas in float64
              that stops, as loops of this kind do, by reading the step size back every iteration.

One process, `--rounds` windows of `--iters` calls between two device events; the report is the median window and the min .. max
spread (the conventions of tools/eval_bench.py).  Needs the GPU: there is no fallback.

    python3 tools/calibration_bench.py [--out profiles/calibration_bench.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from eval_bench import DEV, batch, measure  # noqa: E402
from ood_object_detection_amd.calibration import DetectionCalibrator  # noqa: E402
from ood_object_detection_amd.effdet.evaluation import CalibrationEvaluator, DatasetDetectionEvaluator  # noqa: E402


def fill(ev, n, C, T, seed):
    """n synthetic accumulated detections straight into the evaluator's buffers: uniform classes, float32 scores, true positives with
    probability sigmoid(0.6 logit(p) - 0.5) at the first threshold and at fewer later ones, 3 % ignored, IoU in [0.5, 1)"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    ev.clear()
    scores, classes, flags, iou, state = ev.entries()
    p = torch.rand(n, generator=g, device=DEV).clamp(0.01, 0.99)
    scores[:n] = p
    classes[:n] = torch.randint(0, C, (n,), generator=g, device=DEV, dtype=torch.int32)
    tp = torch.rand(n, generator=g, device=DEV) < torch.sigmoid(0.6 * torch.logit(p.double()) - 0.5).float()
    reach = 1 + (torch.rand(n, generator=g, device=DEV) * T).to(torch.int32)
    word = torch.where(tp, torch.bitwise_left_shift(torch.ones_like(reach), reach) - 1, torch.zeros_like(reach))
    ignored = torch.rand(n, generator=g, device=DEV) < 0.03
    flags[:n] = torch.where(ignored, word << 16, word).to(torch.int32)
    iou[:n] = 0.5 + 0.5 * torch.rand(n, generator=g, device=DEV)
    state[0] = n


def torch_tables(scores, classes, flags, iou, C, K):
    """the pooled and per-class equal-width tables of threshold 0"""
    live = ((flags >> 16) & 1) == 0
    tp = ((flags & 1) == 1) & live
    s, order = torch.sort(scores, descending=True, stable=True)
    c = classes[order].long()
    _, by_class = torch.sort(c, stable=True)
    order = order[by_class]
    p, c, live, tp, u = scores[order].double(), classes[order].long(), live[order], tp[order], iou[order].double()
    edges = torch.arange(1, K, device=DEV, dtype=torch.float32) / K
    k = torch.bucketize(scores[order], edges, right=True)
    out = []
    for cell, cells in ((k, K), (c * K + k, C * K)):
        w = live.double()
        n = torch.zeros(cells, dtype=torch.float64, device=DEV).index_add_(0, cell, w)
        t = torch.zeros(cells, dtype=torch.float64, device=DEV).index_add_(0, cell, tp.double())
        sp = torch.zeros(cells, dtype=torch.float64, device=DEV).index_add_(0, cell, p * w)
        si = torch.zeros(cells, dtype=torch.float64, device=DEV).index_add_(0, cell, u * tp.double())
        out.append((n, t, sp, si))
    return out


def torch_newton(scores, flags, max_iter=32):
    """Platt scaling by Newton's method on the true-positive labels of threshold 0, float64"""
    live = ((flags >> 16) & 1) == 0
    p = scores[live].double().clamp(2.0 ** -24, 1 - 2.0 ** -24)
    x, y = torch.log(p / (1 - p)), (flags[live] & 1).double()
    a, b = 1.0, 0.0
    for it in range(max_iter):
        sg = torch.sigmoid(a * x + b)
        d, w = sg - y, sg * (1 - sg)
        ga, gb, haa, hab, hbb = [float(v) for v in torch.stack([(d * x).sum(), d.sum(), (w * x * x).sum(), (w * x).sum(), w.sum()]).tolist()]
        det = haa * hbb - hab * hab
        da, db = -(hbb * ga - hab * gb) / det, -(haa * gb - hab * ga) / det
        if max(abs(da), abs(db)) <= 2.0 ** -40 * max(1.0, abs(a), abs(b)):
            break
        a, b = a + da, b + db
    return a, b, it + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[65536, 500000, 4000000])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=None, help='also write the report to this file')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'calibration_bench needs the GPU'
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    C, T, K = 80, 10, 15
    cats = [{'id': i + 1, 'name': 'c%d' % i} for i in range(C)]
    thresholds = [round(0.5 + 0.05 * i, 2) for i in range(T)]
    say('CalibrationEvaluator / DetectionCalibrator on %s; C = %d classes, T = %d IoU thresholds, K = %d bins'
        % (torch.cuda.get_device_name(0), C, T, K))
    det, cnt, gtb, gtc, dif, _ = batch(C)
    ev = CalibrationEvaluator(cats, iou_thresholds=thresholds, bins=K, capacity=1 << 23, device=DEV)
    say()
    say('add_batch, %d images x %d detections, %d ground-truth boxes an image:' % (det.shape[0], det.shape[1], gtb.shape[1]))
    old = DatasetDetectionEvaluator(cats, iou_thresholds=thresholds, capacity=1 << 23, device=DEV)
    base = None
    for name, e in (('DatasetDetectionEvaluator: matching + append   ', old), ('CalibrationEvaluator: matching with IoU + append', ev)):
        old.clear(), ev.clear()
        med, lo, hi = measure(lambda: e.add_batch(det, cnt, gtb, gtc, dif), 100, a.rounds)
        base = base or med
        say('  %s median %9.1f us, spread %9.1f .. %9.1f us  (x %.3f)' % (name, med, lo, hi, med / base))
    del ev, old
    for n in a.sizes:
        iters = max(5, min(100, (1 << 24) // n))
        ev = CalibrationEvaluator(cats, iou_thresholds=thresholds, bins=K, capacity=n, device=DEV)
        fill(ev, n, C, T, n)
        scores, classes, flags, iou, _ = ev.entries()
        say()
        say('n = %d accumulated detections:' % n)
        m1 = measure(ev.enqueue, iters, a.rounds)
        say('  enqueue(): 2 sorts, tables of 10 thresholds x 81 scopes x 2 schemes   median %9.1f us, spread %9.1f .. %9.1f us' % m1)
        m0 = measure(lambda: torch_tables(scores, classes, flags, iou, C, K), iters, a.rounds)
        say('  torch: 2 sorts, bucketize, index_add_; 1 threshold, width bins only    median %9.1f us, spread %9.1f .. %9.1f us  (x %.2f)'
            % (m0 + (m0[0] / m1[0],)))
        r = ev.result()
        ref = torch_tables(scores, classes, flags, iou, C, K)[0]
        # (bucketize compares p with float32(k / K), the unit rounds p * K: single entries next to an edge may change bins)
        assert int(ref[0].sum()) == int(r['bins']['n'][0, C, 0].sum()), 'the two disagree on the pooled count'
        cal = DetectionCalibrator('platt', 'tp', DEV)
        f1 = measure(lambda: cal.fit(ev), max(3, iters // 4), a.rounds)
        got = cal.finish()
        say('  fit(): 32 x 2 launches, no host read; converged after %2d evaluations     median %9.1f us, spread %9.1f .. %9.1f us'
            % ((got['iterations'],) + f1))
        f0 = measure(lambda: torch_newton(scores, flags), max(3, iters // 4), a.rounds)
        ta, tb, its = torch_newton(scores, flags)
        say('  torch Newton loop, a host read per iteration, %2d iterations             median %9.1f us, spread %9.1f .. %9.1f us  (x %.2f)'
            % ((its,) + f0 + (f0[0] / f1[0],)))
        say('  (a, b): device %.12f %.12f, torch %.12f %.12f' % (got['a'], got['b'], ta, tb))
        del ev, cal
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
