#!/usr/bin/env python
"""Times of ood_shaping.ActivationShapingOOD (csrc/act_shaping.hip) against the literal torch composition on the same GPU:

  score          of a detection batch ([64, 100] anchor indices: B * K = 6 400 rows) - torch: the depthwise `conv2d` of every level
                 (it has no form that visits selected cells only), a gather of the rows, the shaping written with `clamp` / `topk`,
                 one `linear` per anchor slot through a gathered weight (`bmm`), `logsumexp`, `max`;
  score_anchors  of every anchor - torch: the same `conv2d`, the shaping of every cell, one `linear` to all A * C logits,
                 `logsumexp` and `max` over the classes of each anchor.

Setting: the class tower of d0 / 640 at batch 64 (F = 64, C = 90, A = 9, P = 8 525 cells, N = 76 725 anchors), bfloat16 as the
throughput engine stores it, with seeded values silu(N(0, 1)) and a seeded head; the network itself does not run.  Methods react
(c fitted through the product's own `add` / `fit`) and ash_s at percentile 90.  The paths alternate, `--rounds` windows of
`--iters` calls each between two device events (host launch overhead included); the report is the median window and the
min .. max spread per path.  Needs the GPU.

    python3 tools/act_shaping_bench.py [--out profiles/act_shaping_bench.txt]"""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ood_object_detection_amd.ood_shaping import ActivationShapingOOD  # noqa: E402


def window(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters


class TorchComposition:
    """The same scores in torch ops, from the same float32 head"""

    def __init__(self, s):
        taps, W, bias = (torch.from_numpy(a).to(s.device) for a in (s._head[0], s.weight, s._head[2]))
        self.F, self.C, self.A, self.method, self.k, self.c, self.T = s.F, s.C, s.A, s.method, s.k, s.c, s.temperature
        self.wdw = taps.t().reshape(s.F, 1, 3, 3).contiguous()
        self.W, self.bias = W, bias
        self.Wa, self.ba = W.reshape(s.A, s.C, s.F), bias.reshape(s.A, s.C)

    def d(self, tower):
        B = tower[0].shape[0]
        return torch.cat([torch.nn.functional.conv2d(t.float(), self.wdw, groups=self.F, padding=1).permute(0, 2, 3, 1).reshape(B, -1, self.F)
                          for t in tower], 1)

    def shape(self, d):
        if self.method == 'none':
            return d
        if self.method == 'react':
            return d.clamp(max=self.c)
        pos = d.clamp(min=0)
        s1 = pos.sum(-1, keepdim=True)
        top, idx = torch.topk(d, self.k, -1)
        s2 = top.clamp(min=0).sum(-1, keepdim=True)
        f = torch.where(s2 == 0, torch.ones_like(s2), torch.exp(s1 / s2))
        if self.method == 'scale':
            return d * f
        val = {'ash_p': top, 'ash_b': (s1 / self.k).expand_as(top), 'ash_s': top * f}[self.method]
        return torch.zeros_like(d).scatter_(-1, idx, val)

    def scores(self, z):
        return -self.T * torch.logsumexp(z / self.T, -1), z.max(-1)

    def score(self, tower, anchor, count):
        d = self.d(tower)
        B, K = anchor.shape
        rows = self.shape(d[torch.arange(B, device=d.device)[:, None], anchor // self.A]).reshape(B * K, self.F, 1)
        slot = (anchor % self.A).reshape(-1)
        z = (torch.bmm(self.Wa[slot], rows).squeeze(-1) + self.ba[slot]).reshape(B, K, self.C)
        e, (m, c) = self.scores(z)
        keep = torch.arange(K, device=d.device)[None, :] < count[:, None]
        return torch.where(keep, e, torch.zeros_like(e)), torch.where(keep, m, torch.zeros_like(m)), torch.where(keep, c, torch.full_like(c, -1))

    def score_anchors(self, tower):
        x = self.shape(self.d(tower))
        B, P = x.shape[:2]
        z = torch.nn.functional.linear(x, self.W, self.bias).reshape(B, P * self.A, self.C)
        e, (m, c) = self.scores(z)
        return e, m, c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--out', default=None, help='also write the report to this file')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'act_shaping_bench needs the GPU'
    dev = 'cuda:0'
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    say('ActivationShapingOOD on %s: median microseconds per call of %d windows of %d calls (min .. max), paths alternated'
        % (torch.cuda.get_device_name(0), a.rounds, a.iters))
    F, C, A, B, K, size = 64, 90, 9, 64, 100, 640
    sides = [size // 2 ** l for l in range(3, 8)]
    P = sum(s * s for s in sides)
    N = A * P
    gen = torch.Generator(device=dev).manual_seed(size)
    tower = [torch.nn.functional.silu(torch.randn(B, s, s, F, generator=gen, device=dev)).to(torch.bfloat16).permute(0, 3, 1, 2) for s in sides]
    taps = 0.3 * torch.randn(9, F, generator=gen, device=dev)
    W = torch.randn(A * C, F, generator=gen, device=dev) / math.sqrt(F)
    bias = 0.1 * torch.randn(A * C, generator=gen, device=dev)
    anchor = torch.randint(0, N, (B, K), generator=gen, device=dev)
    count = torch.randint(K // 2, K + 1, (B,), generator=gen, device=dev, dtype=torch.int32)
    say('d0 / 640 / batch %d: F = %d, C = %d, A = %d, P = %d cells, N = %d anchors, bfloat16 tower (%.0f MB); B * K = %d rows'
        % (B, F, C, A, P, N, B * P * F * 2 / 1e6, B * K))
    for method in ('react', 'ash_s'):
        s = ActivationShapingOOD(F, C, A, method=method, percentile=90.0, device=dev)
        s.set_weights(taps.cpu().numpy(), W.cpu().numpy(), bias.cpu().numpy())
        if s.needs_fit:
            s.add(tower, anchor, count)
            s.fit()
        t = TorchComposition(s)
        got, lit = s.score(tower, anchor, count), t.score(tower, anchor, count)
        gota, lita = s.score_anchors([x[:2] for x in tower]), t.score_anchors([x[:2] for x in tower])
        torch.cuda.synchronize()
        say()
        say('%s (k = %d, c = %s)' % (method, s.k, s.c))
        for what, g, l in (('', got, lit), (' of the anchors', gota, lita)):
            for i, key in enumerate(s.KEYS):
                if key.endswith('class'):
                    say('  %s%s: %d of %d differ from torch' % (key, what, int((g[key] != l[i]).sum()), l[i].numel()))
                else:
                    say('  largest |%s%s - torch| %.2e at a largest |value| of %.3g' % (key, what, float((g[key] - l[i]).abs().max()), float(l[i].abs().max())))
        pairs = (('score, detections [%d, %d]' % (B, K), lambda: s.score(tower, anchor, count), lambda: t.score(tower, anchor, count)),
                 ('score_anchors [%d, %d]' % (B, N), lambda: s.score_anchors(tower), lambda: t.score_anchors(tower)))
        for label, new, old in pairs:
            for fn in (new, old):
                window(fn, 2)
            tn, to = [], []
            for _ in range(a.rounds):
                tn.append(window(new, a.iters))
                to.append(window(old, a.iters))
            mn, mo = statistics.median(tn), statistics.median(to)
            say('  %-36s HIP %10.1f us (%10.1f .. %10.1f)   torch %10.1f us (%10.1f .. %10.1f)   ratio torch / HIP %.2f'
                % (label, mn, min(tn), max(tn), mo, min(to), max(to), mo / mn))
        del s, t
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, 'w') as fo:
            fo.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
