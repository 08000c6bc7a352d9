#!/usr/bin/env python
"""Time of the dataset-scale detection evaluation (effdet.evaluation.DatasetDetectionEvaluator, csrc/eval_scale.hip):

  add_batch   one batch of 64 images x 100 detections, 80 classes, 10 IoU thresholds (matching + append, 3 launches);
  enqueue()   sort + AP over n accumulated detections, n = 65 536, 500 000 and 4 000 000, C = 80, T = 10; nothing is read back;
  at n = 65 536 also T = 1 on the sorted path against `effdet_eval_ap`, the rank-counting entry point of the training loop, on
  the same input.  The sorted path must be the faster one there: the tool fails otherwise.

One process, `--rounds` windows of `--iters` calls between two device events; the report is the median window and the min .. max
spread.  Needs the GPU: there is no fallback.

    python3 tools/eval_bench.py [--out profiles/eval_scale_bench.txt]

--openimages: OpenImagesDetectionEvaluator (csrc/openimages_eval.hip) beside DatasetDetectionEvaluator on identical inputs without
group-of boxes - add_batch (its match searches two candidates a detection, and it writes M T virtual slots) and enqueue() at the
same sizes, with and without the pooled AP - and add_batch with 30 % group-of boxes.

    python3 tools/eval_bench.py --openimages [--out profiles/openimages_eval_bench.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ood_object_detection_amd import _lib  # noqa: E402
from ood_object_detection_amd.effdet.evaluation import DatasetDetectionEvaluator  # noqa: E402

DEV = 'cuda:0'


def window(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters


def measure(fn, iters, rounds):
    for _ in range(2):
        window(fn, max(1, iters // 4))
    t = [window(fn, iters) for _ in range(rounds)]
    return statistics.median(t), min(t), max(t)


def fill(ev, n, C, T, seed):
    """n synthetic accumulated detections straight into the evaluator's buffers: uniform classes, float32 scores, about 30 % true
    positives at the first threshold and fewer at every later one, 3 % ignored"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    ev.clear()
    ev._bufs[0][:n] = torch.rand(n, generator=g, device=DEV)
    ev._bufs[1][:n] = torch.randint(0, C, (n,), generator=g, device=DEV, dtype=torch.int32)
    level = (torch.rand(n, generator=g, device=DEV) * 3.3 * T).to(torch.int32)            # thresholds the match reaches
    word = torch.where(level < T, torch.bitwise_left_shift(torch.ones_like(level), (T - level).clamp(min=0)) - 1, torch.zeros_like(level))
    ignored = torch.rand(n, generator=g, device=DEV) < 0.03
    ev._bufs[2][:n] = torch.where(ignored, word << 16, word).to(torch.int32)
    ev._state[0] = n
    ev._gt_count.fill_(max(1, n // (2 * C)))
    ev._gt_imgs.fill_(1)


def batch(C, B=64, D=100, M=16):
    """64 images x 100 detections, 16 ground-truth boxes an image, detections = jittered ground truth"""
    g = torch.Generator(device=DEV).manual_seed(1)
    y0, x0 = torch.rand(B, M, generator=g, device=DEV) * 500, torch.rand(B, M, generator=g, device=DEV) * 500
    gtb = torch.stack([y0, x0, y0 + 40 + 80 * torch.rand(B, M, generator=g, device=DEV), x0 + 40 + 80 * torch.rand(B, M, generator=g, device=DEV)], 2)
    gtc = torch.randint(1, C + 1, (B, M), generator=g, device=DEV)
    pick = torch.randint(0, M, (B, D), generator=g, device=DEV)
    box = torch.gather(gtb, 1, pick[:, :, None].expand(B, D, 4)) + 6 * torch.randn(B, D, 4, generator=g, device=DEV)
    score = torch.sort(torch.rand(B, D, generator=g, device=DEV), 1, descending=True)[0]
    det = torch.stack([box[:, :, 1], box[:, :, 0], box[:, :, 3], box[:, :, 2], score, torch.gather(gtc, 1, pick).float()], 2).contiguous()
    cnt = torch.full((B,), D, dtype=torch.int32, device=DEV)
    dif = (torch.rand(B, M, generator=g, device=DEV) < 0.1).to(torch.uint8)
    grp = ((torch.rand(B, M, generator=g, device=DEV) < 0.3) & (dif == 0)).to(torch.uint8)
    return det, cnt, gtb, gtc, dif, grp


def openimages(a, say, cats, thresholds, C, T):
    from ood_object_detection_amd.effdet.evaluation import OpenImagesDetectionEvaluator
    det, cnt, gtb, gtc, dif, grp = batch(C)
    B, D, M = det.shape[0], det.shape[1], gtb.shape[1]
    say('OpenImagesDetectionEvaluator beside DatasetDetectionEvaluator on %s; C = %d, T = %d' % (torch.cuda.get_device_name(0), C, T))
    say()
    say('add_batch, %d images x %d detections, %d ground-truth boxes an image:' % (B, D, M))
    old = DatasetDetectionEvaluator(cats, iou_thresholds=thresholds, capacity=1 << 23, device=DEV)
    new = OpenImagesDetectionEvaluator(cats, iou_thresholds=thresholds, group_of_weight=1.0, capacity=1 << 23, device=DEV)
    cases = (('DatasetDetectionEvaluator                      ', lambda: old.add_batch(det, cnt, gtb, gtc, dif)),
             ('OpenImages, no group-of table                  ', lambda: new.add_batch(det, cnt, gtb, gtc, gt_difficult=dif)),
             ('OpenImages, 30 % group-of boxes, weight 1       ', lambda: new.add_batch(det, cnt, gtb, gtc, gt_group_of=grp, gt_difficult=dif)))
    base = None
    for name, fn in cases:
        old.clear(), new.clear()
        med, lo, hi = measure(fn, 100, a.rounds)
        base = base or med
        say('  %s median %9.1f us, spread %9.1f .. %9.1f us  (x %.2f)' % (name, med, lo, hi, med / base))
    del old, new
    for n in a.sizes:
        iters = max(5, min(100, (1 << 24) // n))
        say()
        say('n = %d accumulated detections, enqueue():' % n)
        base = None
        for name, make in (('DatasetDetectionEvaluator            ', lambda: DatasetDetectionEvaluator(cats, iou_thresholds=thresholds, capacity=n, device=DEV)),
                           ('OpenImages, per-class AP             ', lambda: OpenImagesDetectionEvaluator(cats, iou_thresholds=thresholds, capacity=n, device=DEV)),
                           ('OpenImages, per-class and pooled AP  ', lambda: OpenImagesDetectionEvaluator(cats, iou_thresholds=thresholds, capacity=n, device=DEV,
                                                                                                      use_weighted_mean_ap=True))):
            ev = make()
            fill(ev, n, C, T, n)
            med, lo, hi = measure(ev.enqueue, iters, a.rounds)
            base = base or med
            r = ev.result()
            say('  %s median %9.1f us, spread %9.1f .. %9.1f us  (x %.2f; mAP@0.5 %.4f)' % (name, med, lo, hi, med / base, float(r['ap'][0].mean())))
            del ev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--openimages', action='store_true', help='time OpenImagesDetectionEvaluator beside DatasetDetectionEvaluator')
    ap.add_argument('--sizes', type=int, nargs='+', default=[65536, 500000, 4000000])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=None, help='also write the report to this file')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'eval_bench needs the GPU'
    lib = _lib.load()
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    C, T = 80, 10
    cats = [{'id': i + 1, 'name': 'c%d' % i} for i in range(C)]
    thresholds = [round(0.5 + 0.05 * i, 2) for i in range(T)]
    if a.openimages:
        openimages(a, say, cats, thresholds, C, T)
        if a.out:
            with open(a.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')
        return
    say('DatasetDetectionEvaluator on %s; C = %d classes, T = %d IoU thresholds (0.50:0.05:0.95)' % (torch.cuda.get_device_name(0), C, T))

    # ---- add_batch
    det, cnt, gtb, gtc, dif, _ = batch(C)
    B, D, M = det.shape[0], det.shape[1], gtb.shape[1]
    ev = DatasetDetectionEvaluator(cats, iou_thresholds=thresholds, capacity=1 << 23, device=DEV)
    flags = ev.add_batch(det, cnt, gtb, gtc, dif)
    say()
    say('add_batch, %d images x %d detections, %d ground-truth boxes an image (%.0f %% true positives at 0.5):'
        % (B, D, M, 100.0 * float((flags & 1).float().mean())))

    def add():
        ev.add_batch(det, cnt, gtb, gtc, dif)
    ev.clear()
    med, lo, hi = measure(add, 100, a.rounds)                               # every call of the run fits the capacity
    say('  matching + append (3 launches)                 median %9.1f us, spread %9.1f .. %9.1f us  (%d windows of 100)' % (med, lo, hi, a.rounds))
    del ev

    # ---- enqueue
    for n in a.sizes:
        ev = DatasetDetectionEvaluator(cats, iou_thresholds=thresholds, capacity=n, device=DEV)
        fill(ev, n, C, T, n)
        iters = max(5, min(100, (1 << 24) // n))
        med, lo, hi = measure(ev.enqueue, iters, a.rounds)
        r = ev.result()
        say()
        say('n = %d accumulated detections: mAP@0.5 %.4f, mAP@0.95 %.4f' % (n, float(r['ap'][0].mean()), float(r['ap'][-1].mean())))
        say('  enqueue(), T = 10 (15 sort + 1 AP launch)       median %9.1f us, spread %9.1f .. %9.1f us  (%d windows of %d)' % (med, lo, hi, a.rounds, iters))
        if n <= 65536:
            one = DatasetDetectionEvaluator(cats, iou_thresholds=(0.5,), capacity=n, device=DEV)
            fill(one, n, C, 1, n)
            m1 = measure(one.enqueue, iters, a.rounds)
            say('  enqueue(), T = 1                                median %9.1f us, spread %9.1f .. %9.1f us' % m1)
            scores, classes = one._bufs[0], one._bufs[1]
            word = one._bufs[2]
            tp = torch.where((word >> 16) & 1 == 1, torch.full_like(word, -1), word & 1).contiguous()
            out = torch.zeros(C, dtype=torch.float64, device=DEV)
            nb = lib.effdet_eval_ap_workspace_bytes(n)
            ws = torch.empty((nb + 7) // 8, dtype=torch.float64, device=DEV)
            st = torch.cuda.current_stream().cuda_stream

            def rank():
                _lib.check(lib.effdet_eval_ap(st, scores.data_ptr(), classes.data_ptr(), tp.data_ptr(), n, C, one._gt_count.data_ptr(),
                                              out.data_ptr(), ws.data_ptr(), nb), 'effdet_eval_ap')
            m0 = measure(rank, 3, a.rounds)
            say('  effdet_eval_ap (rank counting), T = 1           median %9.1f us, spread %9.1f .. %9.1f us' % m0)
            diff = float((out.cpu() - torch.from_numpy(one.result()['ap'][0])).abs().max())
            say('  largest AP difference between the two: %.2e; ratio rank counting / sorted: %.1f' % (diff, m0[0] / m1[0]))
            assert m1[0] < m0[0], 'the sorted path must be faster than rank counting at n = 65 536'
        del ev
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
