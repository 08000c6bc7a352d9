#!/usr/bin/env python
"""Time of the LVIS federated evaluation (effdet.evaluation.LvisDetectionEvaluator, csrc/lvis_eval.hip) on a validation set of LVIS's
shape: 5 000 images x 300 detections, C = 1 203 categories, about 7 boxes an image, per image about 8 categories checked absent
(Kn = 16) and about 1 not exhaustively annotated (Ke = 4), fed as batches of 64; ten IoU thresholds, four area ranges, max_dets
(300,), 101 recall thresholds.

  add_batch   matching + append of one batch (3 launches), the mean over the 79 batches of a pass;
  enqueue()   sort + gather + AP / AR over the accumulated detections of the pass;
  match       the matching launch alone on one batch of 64 (effdet_lvis_match beside effdet_coco_match at equal shapes).

Beside it, on the same tensors (rows in descending score order, which both accept) and in alternated windows:
`CocoDetectionEvaluator(max_dets=(300,))`, which keeps every detection of every category and so accumulates more entries.  The
device result on the first `--ref-images` images is compared with the numpy restatement tests/_lvis_eval_ref.py bit for bit
before anything is timed.  Nothing is read back inside a window.  Nothing here is pass / fail on time.

    python3 tools/lvis_eval_bench.py [--out profiles/lvis_eval_bench.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import _lvis_eval_ref as L  # noqa: E402
from coco_eval_bench import measure_pair  # noqa: E402
from ood_object_detection_amd import _lib  # noqa: E402
from ood_object_detection_amd.effdet.evaluation import CocoDetectionEvaluator, LvisDetectionEvaluator  # noqa: E402

DEV = 'cuda:0'


def make_set(N, D, M, C, Kn, Ke, seed):
    """-> det [N, D, 6] (descending scores), count [N], gt_boxes [N, M, 4], gt_cls [N, M], neg_cls [N, Kn], nel_cls [N, Ke] on the
    device: 1 .. 13 boxes an image with labels from 400 of the C categories; detections = jittered ground truth, half with the
    box's label, a quarter with a label of the image's neg list, the rest any label; nel: labels of the image's detections"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, generator=g, device=DEV)
    ri = lambda lo, hi, *s: torch.randint(lo, hi, s, generator=g, device=DEV)
    labels = torch.randperm(C, generator=g, device=DEV)[:400] + 1
    m = ri(1, 14, N)
    y0, x0 = rnd(N, M) * 480, rnd(N, M) * 480
    side = torch.exp(rnd(N, M) * 3.2 + 2.3)                                   # 10 .. 245 px: small, medium and large boxes
    gtb = torch.stack([y0, x0, y0 + side, x0 + side * (0.5 + rnd(N, M))], 2)
    gtc = labels[ri(0, 400, N, M)]
    gtc = torch.where(torch.arange(M, device=DEV)[None] < m[:, None], gtc, torch.full_like(gtc, -1))
    neg = labels[ri(0, 400, N, Kn)]
    neg = torch.where(torch.arange(Kn, device=DEV)[None] < ri(4, 13, N)[:, None], neg, torch.full_like(neg, -1))
    pick = (rnd(N, D) * m[:, None]).long()
    box = torch.gather(gtb, 1, pick[:, :, None].expand(N, D, 4))
    box = box + 0.08 * (box[:, :, 2:3] - box[:, :, 0:1]) * torch.randn(N, D, 4, generator=g, device=DEV)
    u = rnd(N, D)
    from_neg = torch.gather(neg, 1, ri(0, 4, N, D))                           # the first four entries of a neg list are never padding
    cls = torch.where(u < 0.5, torch.gather(gtc, 1, pick), torch.where(u < 0.75, from_neg, ri(1, C + 1, N, D)))
    nel = torch.gather(cls, 1, ri(0, D, N, Ke))
    nel = torch.where(torch.arange(Ke, device=DEV)[None] < ri(0, 3, N)[:, None], nel, torch.full_like(nel, -1))
    score = torch.sort(rnd(N, D), 1, descending=True)[0]
    det = torch.stack([box[:, :, 1], box[:, :, 0], box[:, :, 3], box[:, :, 2], score, cls.float()], 2).contiguous()
    return det, torch.full((N,), D, dtype=torch.int32, device=DEV), gtb.contiguous(), gtc.contiguous(), neg.contiguous(), nel.contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=5000)
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--ref-images', type=int, default=8)
    ap.add_argument('--out', default=None, help='also write the report to this file')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'lvis_eval_bench needs the GPU'
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    N, B, D, M, C, Kn, Ke = a.images, a.batch, 300, 16, 1203, 16, 4
    cats = [{'id': i + 1, 'name': 'c%d' % i, 'frequency': 'rcf'[i % 3]} for i in range(C)]
    det, cnt, gtb, gtc, neg, nel = make_set(N, D, M, C, Kn, Ke, 1)
    batches = [slice(i, min(i + B, N)) for i in range(0, N, B)]
    lvis = LvisDetectionEvaluator(cats, capacity=N * D, device=DEV)
    coco = CocoDetectionEvaluator(cats, max_dets=(300,), capacity=N * D, device=DEV)
    say('LvisDetectionEvaluator on %s: %d images x %d detections, %d categories, %.1f boxes, %.1f neg and %.1f nel categories an image, '
        'batches of %d' % (torch.cuda.get_device_name(0), N, D, C, float((gtc > 0).sum()) / N, float((neg > 0).sum()) / N,
                           float((nel > 0).sum()) / N, B))

    # ---- the device against the restatement on the CPU
    R = min(a.ref_images, N)
    h = [t[:R].cpu().numpy() for t in (det, gtb, gtc, neg, nel)]
    images = [dict(det_boxes=h[0][i][:, [1, 0, 3, 2]], det_scores=h[0][i][:, 4], det_classes=h[0][i][:, 5].astype(np.int64) - 1,
                   gt_boxes=h[1][i][h[2][i] > 0], gt_classes=h[2][i][h[2][i] > 0] - 1, neg=(h[3][i][h[3][i] > 0] - 1).tolist(),
                   nel=(h[4][i][h[4][i] > 0] - 1).tolist()) for i in range(R)]
    ref = L.evaluate(images, C)
    lvis.add_batch(det[:R], cnt[:R], gtb[:R], gtc[:R], None, neg[:R], nel[:R])
    lvis.enqueue()
    r = lvis.result()
    same = r['n'] == len(ref['scores']) and all(np.array_equal(np.isnan(r[k]), np.isnan(ref[k])) and
                                                np.array_equal(np.nan_to_num(r[k]), np.nan_to_num(ref[k])) for k in ('ap', 'ar'))
    say('  device AP / AR on the first %d images equal to the numpy restatement bit for bit: %s (%d of %d detections kept; the filter '
        'dropped %d, nel ignored %d)' % (R, same, r['n'], R * D, ref['stats']['filtered'], ref['stats']['nel']))
    assert same

    # ---- add_batch: a pass over the whole set
    def feed(ev):
        def run():
            ev.clear()
            for s in batches:
                if ev is lvis:
                    ev.add_batch(det[s], cnt[s], gtb[s], gtc[s], None, neg[s], nel[s])
                else:
                    ev.add_batch(det[s], cnt[s], gtb[s], gtc[s])
        return run
    fmt = '  %-46s median %8.3f ms, spread %8.3f .. %8.3f ms'
    ml, mc = measure_pair(feed(lvis), feed(coco), 1, a.rounds)
    nb = len(batches)
    say()
    say('add_batch, mean over the %d batches of a pass (measured; %d alternated windows of one pass each)' % (nb, a.rounds))
    say(fmt % (('LVIS (rank, cap 300, filter, nel; T 10 x A 4)',) + tuple(v / nb for v in ml)))
    say(fmt % (('CocoDetectionEvaluator (max_dets 300)',) + tuple(v / nb for v in mc)))
    say('  ratio of the medians LVIS / COCO: %.2f' % (ml[0] / mc[0]))

    # ---- the match launch alone, one batch of 64
    lib = _lib.load()
    s = batches[0]
    n = s.stop - s.start
    d, c, gb, gc, ng, nl = (t[s].contiguous() for t in (det, cnt, gtb, gtc, neg, nel))
    flags = torch.empty(n, D, 4, dtype=torch.int32, device=DEV)
    rank, kept = torch.empty(n, D, dtype=torch.int32, device=DEV), torch.empty(2 * n, dtype=torch.int32, device=DEV)
    npig = torch.zeros(C * 4, dtype=torch.int32, device=DEV)
    st = lambda: torch.cuda.current_stream().cuda_stream

    def match_lvis():
        _lib.check(lib.effdet_lvis_match(st(), d.data_ptr(), c.data_ptr(), gb.data_ptr(), gc.data_ptr(), None, n, D, M, C, lvis._thr, 10,
                                         lvis._area_arr, 4, 300, 0.0, ng.data_ptr(), Kn, nl.data_ptr(), Ke, flags.data_ptr(),
                                         rank.data_ptr(), kept.data_ptr(), npig.data_ptr()), 'effdet_lvis_match')

    def match_coco():
        _lib.check(lib.effdet_coco_match(st(), d.data_ptr(), c.data_ptr(), gb.data_ptr(), gc.data_ptr(), None, None, n, D, M, C, lvis._thr,
                                         10, lvis._area_arr, 4, 300, 0.0, flags.data_ptr(), rank.data_ptr(), kept.data_ptr(),
                                         npig.data_ptr()), 'effdet_coco_match')
    ml, mc = measure_pair(match_lvis, match_coco, 20, a.rounds)
    say()
    say('the match launch alone, %d images x %d detections (measured; %d alternated windows of 20 launches)' % (n, D, a.rounds))
    say(fmt % (('effdet_lvis_match (%d B of LDS a workgroup)' % lib.effdet_lvis_match_lds_bytes(D, M, C),) + ml))
    say(fmt % (('effdet_coco_match',) + mc))
    say('  ratio of the medians LVIS / COCO: %.2f' % (ml[0] / mc[0]))

    # ---- enqueue over the accumulated set
    feed(lvis)()
    feed(coco)()
    ml, mc = measure_pair(lvis.enqueue, coco.enqueue, 3, a.rounds)
    out = lvis.evaluate()
    say()
    say('enqueue() (measured; %d alternated windows of 3): LVIS over n = %d kept detections, COCO over n = %d'
        % (a.rounds, lvis.result()['n'], coco.result()['n']))
    say(fmt % (('LVIS (sort + gather + %d-cell AP / AR)' % (C * 10 * 4),) + ml))
    say(fmt % (('CocoDetectionEvaluator (the same cells)',) + mc))
    say('  ratio of the medians LVIS / COCO: %.2f' % (ml[0] / mc[0]))
    say('  AP %.4f, AP50 %.4f, APr %.4f, APc %.4f, APf %.4f, AR@300 %.4f' % tuple(out[k] for k in ('AP', 'AP50', 'APr', 'APc', 'APf', 'AR@300')))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
