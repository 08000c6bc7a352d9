#!/usr/bin/env python
"""Times of ood_features.KNNFeatureOOD (csrc/feature_knn.hip) against the literal torch composition on the same GPU:

  add     of a detection batch ([B, 100] anchor indices with classes) - torch: boolean-mask gather of the rows (which
          synchronises), normalisation, |r|^2, three slice writes at a host cursor;
  score   of the detections and of every cell (`score_cells`) at k = 10 - torch: gather, normalisation, `q @ bank.T` in chunks of
          at most 2^28 distance entries, (|q|^2 + |r|^2) - 2 q.r clamped at 0, `topk(k, largest=False)`.

Settings: the pyramid of d0 / 640 (F = 64, P = 8525) at batch 64 (6400 detections) against banks of 65 536 and 1 048 576 rows and at
batch 8 for `score_cells` (68 200 rows) against 65 536; the pyramid of d4 / 1024 / batch 8 (F = 224, P = 21824, 800 detections)
against 65 536.  Pyramids and banks hold seeded values; the network itself does not run.  The paths alternate, `--rounds`
windows of calls each between two device events (host launch overhead included); the report is the median window and the
min .. max spread per path, and for the HIP score the achieved share of the 155 TFLOP/s float32-MFMA rate counting
2 * rows * M * F operations (every row of the call, the padding beyond `count` included, as the kernel computes them).
Needs the GPU.

    python3 tools/feature_knn_bench.py [--out profiles/feature_knn_bench.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ood_object_detection_amd.ood_features import KNNFeatureOOD  # noqa: E402

PEAK_F32_MFMA = 155e12
CHUNK = 1 << 28


def window(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters


class TorchComposition:
    """The same bank and scores in torch ops"""

    def __init__(self, F, A, capacity, k, dev):
        self.F, self.A, self.k, self.n = F, A, k, 0
        self.bank = torch.zeros(capacity, F, device=dev)
        self.norms = torch.zeros(capacity, device=dev)
        self.classes = torch.zeros(capacity, dtype=torch.int32, device=dev)

    @staticmethod
    def unit(x):
        x = x.float()
        x = x * (1.0 / torch.sqrt(torch.clamp((x * x).sum(-1, keepdim=True), min=1e-24)))
        return x, (x * x).sum(-1)

    def add_detections(self, pyr, anchor, cls, count):
        B, K = anchor.shape
        keep = torch.arange(K, device=pyr.device)[None, :] < count[:, None]
        b = torch.arange(B, device=pyr.device)[:, None].expand(B, K)[keep]
        rows, n2 = self.unit(pyr[b, (anchor // self.A)[keep]])
        n = rows.shape[0]
        self.bank[self.n:self.n + n], self.norms[self.n:self.n + n], self.classes[self.n:self.n + n] = rows, n2, cls[keep].int()
        self.n += n

    def load(self, f):
        self.n = f.M
        self.bank[:f.M], self.norms[:f.M], self.classes[:f.M] = f.rows[:f.M, :f.F], f.norms[:f.M], f.classes[:f.M]

    def score_rows(self, x):
        q, qn = self.unit(x.reshape(-1, self.F))
        bank, bn = self.bank[:self.n], self.norms[:self.n]
        step = max(CHUNK // self.n, 1)
        kth, near = [], []
        for lo in range(0, q.shape[0], step):
            d2 = torch.clamp((qn[lo:lo + step, None] + bn[None, :]) - 2.0 * (q[lo:lo + step] @ bank.T), min=0.0)
            v, i = torch.topk(d2, min(self.k, self.n), dim=1, largest=False)
            kth.append(-v[:, -1])
            near.append(i[:, 0])
        near = torch.cat(near)
        return torch.cat(kth).reshape(x.shape[:-1]), near.reshape(x.shape[:-1]), self.classes[near].reshape(x.shape[:-1])

    def score(self, pyr, anchor):
        B = pyr.shape[0]
        return self.score_rows(pyr[torch.arange(B, device=pyr.device)[:, None], anchor // self.A])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--classes', type=int, default=90)
    ap.add_argument('--k', type=int, default=10)
    ap.add_argument('--out', default=None, help='also write the report to this file')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'feature_knn_bench needs the GPU'
    dev = 'cuda:0'
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    say('KNNFeatureOOD on %s, k = %d: median microseconds per call of %d windows (min .. max), paths alternated' % (torch.cuda.get_device_name(0), a.k, a.rounds))
    C, A, K = a.classes, 9, 100
    # (name, F, image size, batch, bank rows, score the detections / every cell, calls per window)
    settings = (('d0 / 640 / batch 64', 64, 640, 64, 1 << 16, 'det', 10), ('d0 / 640 / batch 64', 64, 640, 64, 1 << 20, 'det', 3),
                ('d4 / 1024 / batch 8', 224, 1024, 8, 1 << 16, 'det', 10), ('d0 / 640 / batch 8', 64, 640, 8, 1 << 16, 'cells', 3))
    for name, F, size, B, M, what, iters in settings:
        P = sum((size // 2 ** l) ** 2 for l in range(3, 8))
        gen = torch.Generator(device=dev).manual_seed(F + M % 1000)
        means = 1.5 * torch.randn(C, F, generator=gen, device=dev) + 0.75
        scales = torch.logspace(0, -1, F, device=dev)
        ycell = torch.randint(0, C, (B, P), generator=gen, device=dev)
        pyr = means[ycell] + torch.randn(B, P, F, generator=gen, device=dev) * scales
        anchor = torch.randint(0, A * P, (B, K), generator=gen, device=dev)
        det_cls = torch.gather(ycell, 1, anchor // A)
        count = torch.randint(K // 2, K + 1, (B,), generator=gen, device=dev, dtype=torch.int32)
        # the bank: M seeded rows of the same distribution, added through the product's own call
        f = KNNFeatureOOD(F, A, M, k=a.k, num_classes=C, device=dev)
        per = 1 << 16
        for lo in range(0, M, per):
            yb = torch.randint(0, C, (1, per), generator=gen, device=dev)
            f.add(means[yb] + torch.randn(1, per, F, generator=gen, device=dev) * scales, yb, (torch.arange(per, device=dev) * A)[None, :])
        f.fit()
        assert f.M == M
        t = TorchComposition(F, A, M, a.k, dev)
        t.load(f)
        if what == 'det':
            got, lit = f.score(pyr, anchor, count), t.score(pyr, anchor)
            keep = torch.arange(K, device=dev)[None, :] < count[:, None]
            rows = B * K
            new, old = (lambda: f.score(pyr, anchor, count)), (lambda: t.score(pyr, anchor))
            label = 'score, detections [%d, %d]' % (B, K)
        else:
            f1 = KNNFeatureOOD(F, 1, M, k=a.k, num_classes=C, device=dev)
            f1._bank, f1.M = f._bank, f.M                              # the same bank, one anchor per cell
            got, lit = f1.score_cells(pyr), t.score_rows(pyr)
            keep = torch.ones(B, P, dtype=torch.bool, device=dev)
            rows = B * P
            new, old = (lambda: f1.score_cells(pyr)), (lambda: t.score_rows(pyr))
            label = 'score_cells [%d, %d]' % (B, P)
        torch.cuda.synchronize()
        diff = float((got['knn'] - lit[0])[keep].abs().max())
        agree = float((got['knn_index'].long() == lit[1])[keep].float().mean())
        say()
        say('%s, F = %d, P = %d, bank of %d rows: largest |knn - torch| %.2e, nearest row agrees on %.4f' % (name, F, P, M, diff, agree))
        pairs = [(label, new, old, iters, 2.0 * rows * M * F)]
        if what == 'det' and M == 1 << 16:
            fa, ta = KNNFeatureOOD(F, A, 1 << 20, k=a.k, num_classes=C, device=dev), TorchComposition(F, A, 1 << 20, a.k, dev)

            def add_new():
                fa.add(pyr, det_cls, anchor, count)

            def add_old():
                ta.add_detections(pyr, anchor, det_cls, count)
            pairs.insert(0, ('add, detections [%d, %d]' % (B, K), add_new, add_old, 20, None))
        for label, new, old, iters, flops in pairs:
            def fresh():
                if flops is None:
                    fa.clear()
                    ta.n = 0
            for fn in (new, old):
                fresh()
                window(fn, 2)
            tn, to = [], []
            for _ in range(a.rounds):
                fresh()
                tn.append(window(new, iters))
                to.append(window(old, iters))
            mn, mo = statistics.median(tn), statistics.median(to)
            rate = '' if flops is None else '   HIP %.1f TFLOP/s, %.1f %% of the float32-MFMA rate' % (flops / mn / 1e6, 100.0 * flops / (mn * 1e-6) / PEAK_F32_MFMA)
            say('  %-30s HIP %10.1f us (%10.1f .. %10.1f)   torch %10.1f us (%10.1f .. %10.1f)   ratio torch / HIP %.2f%s'
                % (label, mn, min(tn), max(tn), mo, min(to), max(to), mo / mn, rate))
        del f, t, pyr
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, 'w') as fo:
            fo.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
