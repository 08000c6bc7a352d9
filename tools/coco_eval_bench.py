#!/usr/bin/env python
"""Time of the COCO-protocol evaluation (effdet.evaluation.CocoDetectionEvaluator, csrc/coco_eval.hip) on a validation set of COCO's
shape: 5 000 images x 100 detections, C = 90 labels of which 80 have ground truth, about 7 boxes an image (3 % crowd), fed as
batches of 64; ten IoU thresholds, four area ranges, max_dets 1 / 10 / 100, 101 recall thresholds.

  add_batch   matching + append of one batch (3 launches), the mean over the 79 batches of a pass;
  enqueue()   sort + gather + AP / AR over the accumulated detections of the pass.

Beside it, on the same tensors and in alternated windows: `DatasetDetectionEvaluator` at the same ten thresholds (the PASCAL
protocol: no crowd regions, no area ranges, no max_dets - the nearest existing yardstick, not the same work).  And the numpy
restatement tests/_coco_eval_ref.py on the CPU over the first `--ref-images` images (the whole set would take minutes); its time
for 5 000 images is EXTRAPOLATED from that, and says so.  The device result on those images is compared with the restatement
bit for bit before anything is timed.  Nothing is read back inside a window.  Nothing here is pass / fail on time.

    python3 tools/coco_eval_bench.py [--out profiles/coco_eval_bench.txt]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import _coco_eval_ref as K  # noqa: E402
from ood_object_detection_amd.effdet.evaluation import CocoDetectionEvaluator, DatasetDetectionEvaluator  # noqa: E402

DEV = 'cuda:0'


def window(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters                                        # ms


def measure_pair(fa, fb, iters, rounds):
    """alternated windows of fa and fb -> ((median, min, max) of fa, of fb), ms"""
    for fn in (fa, fb):
        window(fn, 1)
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(window(fa, iters))
        tb.append(window(fb, iters))
    return (statistics.median(ta), min(ta), max(ta)), (statistics.median(tb), min(tb), max(tb))


def make_set(N, D, M, C, seed):
    """-> det [N, D, 6], count [N], gt_boxes [N, M, 4], gt_cls [N, M] (labels from 80 of the C), gt_crowd [N, M] on the device:
    1 .. 13 boxes an image (7 on average), detections = jittered ground truth (half with the box's label) in descending score"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=g, device=DEV)
    labels = torch.randperm(C, generator=g, device=DEV)[:80] + 1
    m = torch.randint(1, 14, (N,), generator=g, device=DEV)
    y0, x0 = rnd(N, M) * 480, rnd(N, M) * 480
    side = torch.exp(rnd(N, M) * 3.2 + 2.3)                                   # 10 .. 245 px: small, medium and large boxes
    gtb = torch.stack([y0, x0, y0 + side, x0 + side * (0.5 + rnd(N, M))], 2)
    gtc = labels[torch.randint(0, 80, (N, M), generator=g, device=DEV)]
    gtc = torch.where(torch.arange(M, device=DEV)[None] < m[:, None], gtc, torch.full_like(gtc, -1))
    crowd = (rnd(N, M) < 0.03).to(torch.uint8)
    pick = (rnd(N, D) * m[:, None]).long()
    box = torch.gather(gtb, 1, pick[:, :, None].expand(N, D, 4))
    box = box + 0.08 * (box[:, :, 2:3] - box[:, :, 0:1]) * torch.randn(N, D, 4, generator=g, device=DEV)
    cls = torch.gather(gtc, 1, pick)
    cls = torch.where(rnd(N, D) < 0.5, cls, torch.randint(1, C + 1, (N, D), generator=g, device=DEV))
    score = torch.sort(rnd(N, D), 1, descending=True)[0]
    det = torch.stack([box[:, :, 1], box[:, :, 0], box[:, :, 3], box[:, :, 2], score, cls.float()], 2).contiguous()
    return det, torch.full((N,), D, dtype=torch.int32, device=DEV), gtb.contiguous(), gtc.contiguous(), crowd.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=5000)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--ref-images', type=int, default=64)
    ap.add_argument('--out', default=None, help='also write the report to this file')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'coco_eval_bench needs the GPU'
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    N, B, D, M, C = a.images, a.batch, 100, 16, 90
    cats = [{'id': i + 1, 'name': 'c%d' % i} for i in range(C)]
    det, cnt, gtb, gtc, crowd = make_set(N, D, M, C, 1)
    batches = [slice(i, min(i + B, N)) for i in range(0, N, B)]
    coco = CocoDetectionEvaluator(cats, capacity=N * D, device=DEV)
    voc = DatasetDetectionEvaluator(cats, iou_thresholds=[float(np.float32(t)) for t in np.linspace(.5, .95, 10)], capacity=N * D, device=DEV)
    say('CocoDetectionEvaluator on %s: %d images x %d detections, %d labels (80 with ground truth), %.1f boxes an image, batches of %d'
        % (torch.cuda.get_device_name(0), N, D, C, float((gtc > 0).sum()) / N, B))

    # ---- the restatement on the CPU, and the device against it
    R = min(a.ref_images, N)
    host = [t[:R].cpu().numpy() for t in (det, gtb, gtc, crowd)]
    images = [dict(det_boxes=host[0][i][:, [1, 0, 3, 2]], det_scores=host[0][i][:, 4], det_classes=host[0][i][:, 5].astype(np.int64) - 1,
                   gt_boxes=host[1][i][host[2][i] > 0], gt_classes=host[2][i][host[2][i] > 0] - 1, gt_crowd=host[3][i][host[2][i] > 0])
              for i in range(R)]
    t0 = time.perf_counter()
    ref = K.evaluate(images, C)
    t_ref = time.perf_counter() - t0
    coco.add_batch(det[:R], cnt[:R], gtb[:R], gtc[:R], crowd[:R])
    coco.enqueue()
    r = coco.result()
    same = np.array_equal(np.isnan(r['ap']), np.isnan(ref['ap'])) and np.array_equal(np.nan_to_num(r['ap']), np.nan_to_num(ref['ap'])) \
        and np.array_equal(np.nan_to_num(r['ar']), np.nan_to_num(ref['ar']))
    say('numpy restatement on the CPU, %d images: %.2f s = %.1f ms an image (measured); for %d images %.0f s (EXTRAPOLATED, not measured)'
        % (R, t_ref, 1e3 * t_ref / R, N, t_ref / R * N))
    say('  device AP / AR on those images equal to the restatement bit for bit: %s' % same)
    assert same

    # ---- add_batch: a pass over the whole set
    def feed(ev):
        def run():
            ev.clear()
            for s in batches:
                if ev is coco:
                    ev.add_batch(det[s], cnt[s], gtb[s], gtc[s], crowd[s])
                else:
                    ev.add_batch(det[s], cnt[s], gtb[s], gtc[s])
        return run
    fmt = '  %-44s median %8.3f ms, spread %8.3f .. %8.3f ms'
    mc, mv = measure_pair(feed(coco), feed(voc), 1, a.rounds)
    nb = len(batches)
    say()
    say('add_batch, mean over the %d batches of a pass (measured; %d alternated windows of one pass each)' % (nb, a.rounds))
    say(fmt % (('COCO (T 10 x A 4, crowd, ranks)',) + tuple(v / nb for v in mc)))
    say(fmt % (('DatasetDetectionEvaluator (T 10)',) + tuple(v / nb for v in mv)))
    say('  ratio of the medians COCO / PASCAL: %.2f; a d0 batch of 64 takes 3.9 ms (README: 16.6 k img/s): add_batch is %.1f %% of it'
        % (mc[0] / mv[0], 100.0 * mc[0] / nb / 3.9))

    # ---- enqueue over the accumulated set
    feed(coco)()
    feed(voc)()
    mc, mv = measure_pair(coco.enqueue, voc.enqueue, 3, a.rounds)
    r = coco.evaluate()
    say()
    say('enqueue() over n = %d accumulated detections (measured; %d alternated windows of 3)' % (coco.result()['n'], a.rounds))
    say(fmt % (('COCO (sort + gather + %d-cell AP / AR)' % (C * 10 * 4 * 3),) + mc))
    say(fmt % (('DatasetDetectionEvaluator (sort + AP)',) + mv))
    say('  ratio of the medians COCO / PASCAL: %.2f' % (mc[0] / mv[0]))
    say('  stats[0] = mAP@[.5:.95] %.4f, AP50 %.4f, AR100 %.4f' % (r['stats'][0], r['stats'][1], r['stats'][8]))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
