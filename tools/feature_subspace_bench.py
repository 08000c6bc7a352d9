#!/usr/bin/env python
"""Times of ood_features.SubspaceFeatureOOD (csrc/feature_subspace.hip) against the literal torch composition on the same GPU:

  score        of a detection batch ([B, 100] anchor indices, with the logit score, so all three keys) - torch: gather of the rows,
               subtraction of mu0, one float32 `matmul` with R, two reductions (sum y^2 -> sqrt, sum inv_lambda y^2), the vim
               arithmetic, masking beyond `count`;
  score_cells  of every cell - torch: the same without the gather and vim.

Settings: the pyramid of d0 / 640 (F = 64, P = 8525) at batch 64 (6400 detections; 545 600 cells) and of d4 / 1024 / batch 8
(F = 224, P = 21824, 800 detections; 174 592 cells), each at the default D = F // 2 and at D = 0 (every direction).  Pyramids
hold seeded values and the statistics are added through the product's own call; the network itself does not run.  The paths
alternate, `--rounds` windows of calls each between two device events (host launch overhead included); the report is the median
window and the min .. max spread per path, and for the HIP path the achieved share of the 155 TFLOP/s float32-MFMA rate counting
2 * rows * Rp * Fp operations (every row of the call, the padding beyond `count` included, as the kernel computes them).
Needs the GPU.

    python3 tools/feature_subspace_bench.py [--out profiles/feature_subspace_bench.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ood_object_detection_amd.ood_features import SubspaceFeatureOOD  # noqa: E402

PEAK_F32_MFMA = 155e12


def window(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters


class TorchComposition:
    """The same scores in torch ops, from the same uploaded parameters"""

    def __init__(self, f):
        Rt, il, mu0 = f._dev
        Rn = f.F - f.dim
        self.A, self.alpha = f.A, f.alpha
        self.R, self.il, self.mu0 = Rt[:Rn, :f.F].t().contiguous(), il[:Rn].contiguous(), mu0[:f.F].contiguous()

    def rows(self, x):
        y = (x.float() - self.mu0) @ self.R
        y2 = y * y
        return torch.sqrt(y2.sum(-1)), (y2 * self.il).sum(-1)

    def score(self, pyr, anchor, count, energy):
        B, K = anchor.shape
        r, pm = self.rows(pyr[torch.arange(B, device=pyr.device)[:, None], anchor // self.A])
        keep = torch.arange(K, device=pyr.device)[None, :] < count[:, None]
        zero = torch.zeros_like(r)
        return torch.where(keep, -r, zero), torch.where(keep, -pm, zero), torch.where(keep, -energy - self.alpha * r, zero)

    def score_cells(self, pyr):
        r, pm = self.rows(pyr)
        return -r, -pm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--classes', type=int, default=90)
    ap.add_argument('--out', default=None, help='also write the report to this file')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'feature_subspace_bench needs the GPU'
    dev = 'cuda:0'
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    say('SubspaceFeatureOOD on %s: median microseconds per call of %d windows (min .. max), paths alternated' % (torch.cuda.get_device_name(0), a.rounds))
    C, A, K = a.classes, 9, 100
    for name, F, size, B in (('d0 / 640 / batch 64', 64, 640, 64), ('d4 / 1024 / batch 8', 224, 1024, 8)):
        P = sum((size // 2 ** l) ** 2 for l in range(3, 8))
        gen = torch.Generator(device=dev).manual_seed(F)
        means = 1.5 * torch.randn(C, F, generator=gen, device=dev) + 0.75
        scales = torch.logspace(0, -1, F, device=dev)
        ycell = torch.randint(0, C, (B, P), generator=gen, device=dev)
        pyr = means[ycell] + torch.randn(B, P, F, generator=gen, device=dev) * scales
        anchor = torch.randint(0, A * P, (B, K), generator=gen, device=dev)
        count = torch.randint(K // 2, K + 1, (B,), generator=gen, device=dev, dtype=torch.int32)
        energy = -(2.0 + torch.randn(B, K, generator=gen, device=dev))
        f = SubspaceFeatureOOD(F, C, A, device=dev)
        f.add(pyr[:1], ycell[:1].repeat_interleave(A, 1))                 # one image's anchors, the dense form
        for dim in (F // 2, 0):
            f.fit(dim=dim)
            f.calibrate(pyr, anchor, count, energy)
            f.finish_calibration()
            f.reset_calibration()
            t = TorchComposition(f)
            Rp, Fp = f._dev[0].shape
            say()
            say('%s, F = %d, P = %d, D = %d (Rp = %d), alpha %.4f' % (name, F, P, dim, Rp, f.alpha))
            got, lit = f.score(pyr, anchor, count, logit_score=energy), t.score(pyr, anchor, count, energy)
            gotc, litc = f.score_cells(pyr), t.score_cells(pyr)
            torch.cuda.synchronize()
            for key, g, l in (('residual', got['residual'], lit[0]), ('partial_mahalanobis', got['partial_mahalanobis'], lit[1]),
                              ('vim', got['vim'], lit[2]), ('residual of the cells', gotc['residual'], litc[0]),
                              ('partial_mahalanobis of the cells', gotc['partial_mahalanobis'], litc[1])):
                say('  largest |%s - torch| %.2e at a largest |value| of %.3g' % (key, float((g - l).abs().max()), float(l.abs().max())))
            pairs = (('score, detections [%d, %d]' % (B, K), lambda: f.score(pyr, anchor, count, logit_score=energy),
                      lambda: t.score(pyr, anchor, count, energy), 20, B * K),
                     ('calibrate, detections [%d, %d]' % (B, K), lambda: f.calibrate(pyr, anchor, count, energy), None, 20, B * K),
                     ('score_cells [%d, %d]' % (B, P), lambda: f.score_cells(pyr), lambda: t.score_cells(pyr), 5, B * P))
            for label, new, old, iters, rows in pairs:
                for fn in (new, old):
                    if fn is not None:
                        window(fn, 2)
                tn, to = [], []
                for _ in range(a.rounds):
                    tn.append(window(new, iters))
                    if old is not None:
                        to.append(window(old, iters))
                mn = statistics.median(tn)
                flops = 2.0 * rows * Rp * Fp
                rate = 'HIP %.2f TFLOP/s, %.2f %% of the float32-MFMA rate' % (flops / mn / 1e6, 100.0 * flops / (mn * 1e-6) / PEAK_F32_MFMA)
                if old is None:
                    say('  %-34s HIP %9.1f us (%9.1f .. %9.1f)   (no torch counterpart timed)   %s' % (label, mn, min(tn), max(tn), rate))
                else:
                    mo = statistics.median(to)
                    say('  %-34s HIP %9.1f us (%9.1f .. %9.1f)   torch %9.1f us (%9.1f .. %9.1f)   ratio torch / HIP %.2f   %s'
                        % (label, mn, min(tn), max(tn), mo, min(to), max(to), mo / mn, rate))
        del f, t, pyr
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, 'w') as fo:
            fo.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
