#!/usr/bin/env python
"""Times of ood_features.FeatureOOD (csrc/feature_ood.hip) against the literal torch composition on the same GPU:

  add     on a detection batch ([B, 100] anchor indices with classes) and on a dense label batch ([B, A * P] labels, 1 % of them
          positive) - torch: gather of the rows, float64 `index_add_` for s_c / n_c and `x.T @ x` for S (the dense form finds its
          rows with `nonzero`, which synchronises);
  score   of the detections and of every cell (`score_cells`) - torch: gather, three float32 `torch.matmul`, min / argmin.

Settings: the pyramid of d0 / 640 / batch 64 / C = 90 (F = 64, P = 8525) and of d4 / 1024 / batch 8 / C = 90 (F = 224, P = 21824),
filled with seeded values; the network itself does not run.  The paths alternate, `--rounds` windows of `--iters` calls each
between two device events; the report is the median window and the min .. max spread per path.  Needs the GPU.

    python3 tools/feature_ood_bench.py [--out profiles/feature_ood_bench.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ood_object_detection_amd.ood_features import FeatureOOD  # noqa: E402

SETTINGS = (('d0 / 640 / batch 64', 64, 640, 64), ('d4 / 1024 / batch 8', 224, 1024, 8))


def window(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters


class TorchComposition:
    """The same statistics and scores in torch ops"""

    def __init__(self, F, C, A, dev):
        self.F, self.C, self.A = F, C, A
        self.n_c = torch.zeros(C, dtype=torch.int64, device=dev)
        self.s_c = torch.zeros(C, F, dtype=torch.float64, device=dev)
        self.S = torch.zeros(F, F, dtype=torch.float64, device=dev)

    def _accumulate(self, rows, cls):
        x = rows.double()
        self.n_c.index_add_(0, cls, torch.ones_like(cls))
        self.s_c.index_add_(0, cls, x)
        self.S += x.T @ x

    def add_detections(self, pyr, anchor, cls, count):
        B, K = anchor.shape
        keep = torch.arange(K, device=pyr.device)[None, :] < count[:, None]
        b = torch.arange(B, device=pyr.device)[:, None].expand(B, K)[keep]
        self._accumulate(pyr[b, (anchor // self.A)[keep]], cls[keep])

    def add_dense(self, pyr, labels):
        b, n = torch.nonzero(labels >= 0, as_tuple=True)
        self._accumulate(pyr[b, n // self.A], labels[b, n])

    def load(self, f):
        dev = self.S.device
        p = f.params
        self.W, self.W0, self.M = (torch.from_numpy(p[k]).float().to(dev) for k in ('W', 'W0', 'M'))
        self.m2, self.mu0 = torch.from_numpy(p['m2']).float().to(dev), torch.from_numpy(p['mu0']).float().to(dev)

    def score_rows(self, x):
        xc = x.float() - self.mu0
        z, z0 = torch.matmul(xc, self.W.T), torch.matmul(xc, self.W0.T)
        q, d0 = (z * z).sum(-1), (z0 * z0).sum(-1)
        d = (q[..., None] - 2.0 * torch.matmul(z, self.M.T)) + self.m2
        dmin, near = d.min(-1)
        return -dmin, -(dmin - d0), near

    def score(self, pyr, anchor):
        B = pyr.shape[0]
        return self.score_rows(pyr[torch.arange(B, device=pyr.device)[:, None], anchor // self.A])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--classes', type=int, default=90)
    ap.add_argument('--out', default=None, help='also write the report to this file')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'feature_ood_bench needs the GPU'
    dev = 'cuda:0'
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    say('FeatureOOD on %s: median microseconds per call of %d windows of %d calls (min .. max), paths alternated' % (torch.cuda.get_device_name(0), a.rounds, a.iters))
    C, A, K = a.classes, 9, 100
    for name, F, size, B in SETTINGS:
        P = sum((size // 2 ** l) ** 2 for l in range(3, 8))
        gen = torch.Generator(device=dev).manual_seed(F)
        means = 1.5 * torch.randn(C, F, generator=gen, device=dev) + 0.75
        ycell = torch.randint(0, C, (B, P), generator=gen, device=dev)
        scales = torch.logspace(0, -1, F, device=dev)
        for dtype in (torch.float32, torch.bfloat16):
            pyr = (means[ycell] + torch.randn(B, P, F, generator=gen, device=dev) * scales).to(dtype)
            anchor = torch.randint(0, A * P, (B, K), generator=gen, device=dev)
            det_cls = torch.gather(ycell, 1, anchor // A)
            count = torch.randint(K // 2, K + 1, (B,), generator=gen, device=dev, dtype=torch.int32)
            labels = torch.where(torch.rand(B, A * P, generator=gen, device=dev) < 0.01, ycell.repeat_interleave(A, 1), torch.full((B, A * P), -1, device=dev))
            f, t = FeatureOOD(F, C, A, dev), TorchComposition(F, C, A, dev)
            f.add(pyr, labels)
            t.add_dense(pyr, labels)
            torch.cuda.synchronize()
            dS = float((f.S - t.S).abs().max() / t.S.abs().max())
            assert torch.equal(f.n_c, t.n_c) and dS <= 1e-12, dS
            f.fit()
            t.load(f)
            got, lit = f.score(pyr, anchor, count), t.score(pyr, anchor)
            keep = torch.arange(K, device=dev)[None, :] < count[:, None]
            dev_diff = float((got['mahalanobis'] - lit[0])[keep].abs().max())
            agree = float((got['nearest_class'].long() == lit[2])[keep].float().mean())
            say()
            say('%s, C = %d, F = %d, P = %d, %s features: %d rows fitted; largest |mahalanobis - torch| over the detections %.2e, nearest class agrees on %.4f'
                % (name, C, F, P, str(dtype).replace('torch.', ''), int(f.n_c.sum()), dev_diff, agree))
            pairs = [
                ('add, detections [%d, %d]' % (B, K), lambda: f.add(pyr, det_cls, anchor, count), lambda: t.add_detections(pyr, anchor, det_cls, count)),
                ('add, dense labels [%d, %d]' % (B, A * P), lambda: f.add(pyr, labels), lambda: t.add_dense(pyr, labels)),
                ('score, detections [%d, %d]' % (B, K), lambda: f.score(pyr, anchor, count), lambda: t.score(pyr, anchor)),
                ('score_cells [%d, %d]' % (B, P), lambda: f.score_cells(pyr), lambda: t.score_rows(pyr)),
            ]
            for what, new, old in pairs:
                for fn in (new, old):
                    window(fn, 3)
                tn, to = [], []
                for _ in range(a.rounds):
                    tn.append(window(new, a.iters))
                    to.append(window(old, a.iters))
                say('  %-34s HIP %9.1f us (%9.1f .. %9.1f)   torch %9.1f us (%9.1f .. %9.1f)   ratio torch / HIP %.2f'
                    % (what, statistics.median(tn), min(tn), max(tn), statistics.median(to), min(to), max(to),
                       statistics.median(to) / statistics.median(tn)))
    if a.out:
        with open(a.out, 'w') as fo:
            fo.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
