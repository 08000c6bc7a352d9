#!/usr/bin/env python
"""Time of the open-set detection evaluation (effdet.evaluation.OpenSetDetectionEvaluator, csrc/eval_scale.hip) beside the
closed-set path for the same detections, `DatasetDetectionEvaluator` with C + 1 categories:

  add_batch   one batch of 64 images x 100 detections, C = 90 known classes, 32 ground-truth boxes an image of which 8 unknown
              (open set: matching + open words + append, 4 launches; closed set: matching + append, 3 launches);
  enqueue()   sort + AP (+ the open-set counts) over n accumulated detections, n = 100 000 and 2^22;
  both at T = 1 and T = 10 IoU thresholds.  Nothing is read back inside a window.

One process; after a warm-up the windows of the two evaluators alternate, `--rounds` windows each between two device events; the
report is the median window and the min .. max spread, and the ratio of the medians.  Needs the GPU: there is no fallback.

    python3 tools/eval_open_bench.py [--out profiles/eval_open_bench.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ood_object_detection_amd.effdet.evaluation import DatasetDetectionEvaluator, OpenSetDetectionEvaluator  # noqa: E402

DEV = 'cuda:0'


def window(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters


def measure_pair(fa, fb, iters, rounds):
    """alternated windows of fa and fb -> ((median, min, max) of fa, of fb)"""
    for fn in (fa, fb, fa, fb):
        window(fn, max(1, iters // 4))
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(window(fa, iters))
        tb.append(window(fb, iters))
    return (statistics.median(ta), min(ta), max(ta)), (statistics.median(tb), min(tb), max(tb))


def fill(ev, n, C1, T, seed, open_words):
    """n synthetic accumulated detections straight into the evaluator's buffers (tools/eval_bench.py::fill): uniform classes over
    the C + 1, about 30 % true positives at the first threshold and fewer at every later one, 3 % ignored; 10 % open at the first
    threshold"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    ev.clear()
    ev._bufs[0][:n] = torch.rand(n, generator=g, device=DEV)
    ev._bufs[1][:n] = torch.randint(0, C1, (n,), generator=g, device=DEV, dtype=torch.int32)
    level = (torch.rand(n, generator=g, device=DEV) * 3.3 * T).to(torch.int32)
    word = torch.where(level < T, torch.bitwise_left_shift(torch.ones_like(level), (T - level).clamp(min=0)) - 1, torch.zeros_like(level))
    ignored = torch.rand(n, generator=g, device=DEV) < 0.03
    ev._bufs[2][:n] = torch.where(ignored, word << 16, word).to(torch.int32)
    if open_words:
        lv = (torch.rand(n, generator=g, device=DEV) * 10 * T).to(torch.int32)
        w = torch.where(lv < T, torch.bitwise_left_shift(torch.ones_like(lv), (T - lv).clamp(min=0)) - 1, torch.zeros_like(lv))
        ev._open[:n] = torch.where(ev._bufs[1][:n] < C1 - 1, w, torch.zeros_like(w)).to(torch.int32)
    ev._state[0] = n
    ev._gt_count.fill_(max(1, n // (2 * C1)))
    ev._gt_imgs.fill_(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[100000, 1 << 22])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=None, help='also write the report to this file')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'eval_open_bench needs the GPU'
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    C = 90
    known = [{'id': i + 1, 'name': 'c%d' % i} for i in range(C)]
    closed_cats = known + [{'id': C + 1, 'name': 'u'}]
    say('OpenSetDetectionEvaluator beside DatasetDetectionEvaluator(C + 1) on %s; C = %d known classes' % (torch.cuda.get_device_name(0), C))
    fmt = '  %-34s median %9.1f us, spread %9.1f .. %9.1f us'

    # ---- add_batch: 64 images x 100 detections, 32 ground-truth boxes an image (8 unknown), detections = jittered ground truth
    B, D, M, MU = 64, 100, 32, 8
    g = torch.Generator(device=DEV).manual_seed(1)
    y0, x0 = torch.rand(B, M, generator=g, device=DEV) * 500, torch.rand(B, M, generator=g, device=DEV) * 500
    gtb = torch.stack([y0, x0, y0 + 40 + 80 * torch.rand(B, M, generator=g, device=DEV), x0 + 40 + 80 * torch.rand(B, M, generator=g, device=DEV)], 2)
    gtc = torch.randint(1, C + 1, (B, M), generator=g, device=DEV)
    gtc[:, :MU] = C + 1
    pick = torch.randint(0, M, (B, D), generator=g, device=DEV)
    box = torch.gather(gtb, 1, pick[:, :, None].expand(B, D, 4)) + 6 * torch.randn(B, D, 4, generator=g, device=DEV)
    score = torch.sort(torch.rand(B, D, generator=g, device=DEV), 1, descending=True)[0]
    cls = torch.gather(gtc, 1, pick)
    cls = torch.where(torch.rand(B, D, generator=g, device=DEV) < 0.5, cls, torch.randint(1, C + 1, (B, D), generator=g, device=DEV))
    det = torch.stack([box[:, :, 1], box[:, :, 0], box[:, :, 3], box[:, :, 2], score, cls.float()], 2).contiguous()
    cnt = torch.full((B,), D, dtype=torch.int32, device=DEV)
    dif = (torch.rand(B, M, generator=g, device=DEV) < 0.1).to(torch.uint8)
    for T in (1, 10):
        thresholds = [round(0.5 + 0.05 * i, 2) for i in range(T)]
        ev = OpenSetDetectionEvaluator(known, iou_thresholds=thresholds, capacity=1 << 23, device=DEV)
        cl = DatasetDetectionEvaluator(closed_cats, iou_thresholds=thresholds, capacity=1 << 23, device=DEV)
        flags, words = ev.add_batch(det, cnt, gtb, gtc, dif)
        say()
        say('add_batch, T = %d: %d images x %d detections, %d ground-truth boxes an image, %d unknown (%.0f %% true positives, %.0f %% open '
            'at 0.5); %d windows of 100' % (T, B, D, M, MU, 100.0 * float((flags & 1).float().mean()), 100.0 * float((words & 1).float().mean()),
                                         a.rounds))
        ev.clear()
        cl.clear()
        mo, mc = measure_pair(lambda: ev.add_batch(det, cnt, gtb, gtc, dif), lambda: cl.add_batch(det, cnt, gtb, gtc, dif), 100, a.rounds)
        say(fmt % (('open set (4 launches)',) + mo))
        say(fmt % (('closed set, C + 1 (3 launches)',) + mc))
        say('  ratio of the medians open / closed: %.2f' % (mo[0] / mc[0]))
        del ev, cl

    # ---- enqueue
    for n in a.sizes:
        for T in (1, 10):
            thresholds = [round(0.5 + 0.05 * i, 2) for i in range(T)]
            ev = OpenSetDetectionEvaluator(known, iou_thresholds=thresholds, capacity=n, device=DEV)
            cl = DatasetDetectionEvaluator(closed_cats, iou_thresholds=thresholds, capacity=n, device=DEV)
            fill(ev, n, C + 1, T, n, True)
            fill(cl, n, C + 1, T, n, False)
            iters = max(5, min(100, (1 << 24) // n))
            mo, mc = measure_pair(ev.enqueue, cl.enqueue, iters, a.rounds)
            r, rc = ev.result(), cl.result()
            same = bool((r['block'][:len(rc['block'])] == rc['block']).all())
            say()
            say('enqueue(), n = %d accumulated detections, T = %d (AP block equal to the closed set bit for bit: %s; WI@0.5 %.4f, A-OSE@0.5 %d); '
                '%d windows of %d' % (n, T, same, float(r['wi'][0]), int(r['a_ose'][0]), a.rounds, iters))
            say(fmt % (('open set (sort + AP + counts)',) + mo))
            say(fmt % (('closed set, C + 1 (sort + AP)',) + mc))
            say('  ratio of the medians open / closed: %.2f' % (mo[0] / mc[0]))
            assert same
            del ev, cl
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
