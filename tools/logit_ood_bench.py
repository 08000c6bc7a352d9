#!/usr/bin/env python
"""Times of ood_logits.LogitOOD (csrc/logit_ood.hip) against the literal torch composition on the same GPU:

  score          of a detection batch ([B, 100] anchor indices, all eight keys) - torch: gather of the rows, `log_softmax`, `topk`,
                 the literal p^gamma (1 - p)^gamma, `softplus`, one float32 `matmul` with log D, `min`, masking beyond `count`;
  score_anchors  of every anchor - torch: the same without the gather;
  add            in both forms (indexed detections; every anchor whose max logit is at least 4, about 4 % of them) - torch: `log_softmax`, `argmax`
                 and `index_add_` into float64 statistics.

Settings: the class logits of d0 / 640 at batch 64 (C = 90, N = 76 725: 884 MB of bfloat16) and of d4 / 1024 at batch 8
(N = 196 416), bfloat16 as the throughput engine stores them.  Logits hold seeded values (2 N(0, 1) - 3, +5 on one class of
every eighth anchor) and the statistics are added through the product's own call; the network itself does not run.  The paths
alternate, `--rounds` windows of `--iters` calls each between two device events (host launch overhead included); the report is the
median window and the min .. max spread per path, and for the HIP path the achieved bytes per second of logits read against the
8 TB/s HBM peak.  Needs the GPU.

    python3 tools/logit_ood_bench.py [--out profiles/logit_ood_bench.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ood_object_detection_amd.ood_logits import LogitOOD  # noqa: E402

PEAK_HBM = 8e12


def window(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters


class TorchComposition:
    """The same scores and statistics in torch ops, from the same uploaded parameters"""

    def __init__(self, f):
        C = f.C
        log_d, kl_inf, mu, isg = f._dev
        self.C, self.T, self.gamma, self.m = C, f.temperature, f.gamma, min(f.top_m, C)
        self.log_d_t, self.kl_inf, self.mu, self.isg = log_d[:C, :C].t().contiguous(), kl_inf[:C].contiguous(), mu, isg
        dev = log_d.device
        self.n_c = torch.zeros(C, dtype=torch.int64, device=dev)
        self.P_c = torch.zeros(C, C, dtype=torch.float64, device=dev)
        self.a_c, self.b_c = torch.zeros(C, dtype=torch.float64, device=dev), torch.zeros(C, dtype=torch.float64, device=dev)

    def rows(self, z):
        z = z.float()
        l1 = torch.log_softmax(z, -1)
        l = l1 if self.T == 1.0 else torch.log_softmax(z / self.T, -1)
        p = l.exp()
        lm, pred = l.max(-1)
        pt = torch.topk(l, self.m, -1).values.exp()
        gen = -(pt ** self.gamma * (1.0 - pt) ** self.gamma).sum(-1)
        p1 = l1.exp()
        kl = (p1 * l1).sum(-1, keepdim=True) - p1 @ self.log_d_t + self.kl_inf
        klv, klc = kl.min(-1)
        sml = (z.max(-1).values - self.mu[pred]) * self.isg[pred]
        return {'msp': lm.exp(), 'neg_entropy': (p * l).sum(-1), 'gen': gen, 'joint_energy': torch.nn.functional.softplus(z).sum(-1),
                'predicted_class': pred, 'kl_matching': -klv, 'kl_class': klc, 'standardized_max_logit': sml}

    def score(self, logits, anchor, count):
        B, K = anchor.shape
        out = self.rows(logits[torch.arange(B, device=logits.device)[:, None], anchor])
        keep = torch.arange(K, device=logits.device)[None, :] < count[:, None]
        return {k: torch.where(keep, v, torch.full_like(v, -1 if k.endswith('class') else 0)) for k, v in out.items()}

    def add(self, z, keep=None, min_max=None):
        z = z.float().reshape(-1, self.C)
        mz, pred = z.max(-1)
        if min_max is not None:
            keep = mz >= min_max
        if keep is not None:
            keep = keep.reshape(-1)
            z, mz, pred = z[keep], mz[keep], pred[keep]
        self.n_c.index_add_(0, pred, torch.ones_like(pred))
        self.P_c.index_add_(0, pred, torch.softmax(z, -1).double())
        self.a_c.index_add_(0, pred, mz.double())
        self.b_c.index_add_(0, pred, mz.double() ** 2)

    def add_indexed(self, logits, anchor, count):
        B, K = anchor.shape
        self.add(logits[torch.arange(B, device=logits.device)[:, None], anchor], torch.arange(K, device=logits.device)[None, :] < count[:, None])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--classes', type=int, default=90)
    ap.add_argument('--out', default=None, help='also write the report to this file')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'logit_ood_bench needs the GPU'
    dev = 'cuda:0'
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    say('LogitOOD on %s: median microseconds per call of %d windows of %d calls (min .. max), paths alternated' % (torch.cuda.get_device_name(0), a.rounds, a.iters))
    C, A, K = a.classes, 9, 100
    for name, size, B in (('d0 / 640 / batch 64', 640, 64), ('d4 / 1024 / batch 8', 1024, 8)):
        N = A * sum((size // 2 ** l) ** 2 for l in range(3, 8))
        gen = torch.Generator(device=dev).manual_seed(size)
        logits = torch.empty(B, N, C, dtype=torch.bfloat16, device=dev)
        for b in range(B):                                                  # per image: the float32 draw of the whole batch is 1.8 GB
            z = 2.0 * torch.randn(N, C, generator=gen, device=dev) - 3.0
            hot = torch.randint(0, C, (N,), generator=gen, device=dev)
            z[torch.arange(0, N, 8, device=dev), hot[::8]] += 5.0
            logits[b] = z.to(torch.bfloat16)
        del z, hot
        anchor = torch.randint(0, N, (B, K), generator=gen, device=dev)
        count = torch.randint(K // 2, K + 1, (B,), generator=gen, device=dev, dtype=torch.int32)
        f = LogitOOD(C, device=dev)
        f.add(logits[:1], min_max_logit=4.0)                                # one image's confident anchors, the dense form
        f.fit()
        torch.cuda.synchronize()
        t = TorchComposition(f)
        say()
        say('%s, C = %d, N = %d, bfloat16 logits (%.0f MB), %d fit rows' % (name, C, N, logits.numel() * 2 / 1e6, int(f.n_c.sum())))
        got, lit = f.score(logits, anchor, count), t.score(logits, anchor, count)
        gota, lita = f.score_anchors(logits[:2]), t.rows(logits[:2])
        torch.cuda.synchronize()
        for k in f.KEYS:
            for what, g, l in (('', got[k], lit[k]), (' of the anchors', gota[k], lita[k])):
                if k.endswith('class'):
                    say('  %s%s: %d of %d differ from torch' % (k, what, int((g != l).sum()), g.numel()))
                else:
                    say('  largest |%s%s - torch| %.2e at a largest |value| of %.3g' % (k, what, float((g - l).abs().max()), float(l.abs().max())))
        thr = 4.0
        pairs = (('score, detections [%d, %d]' % (B, K), lambda: f.score(logits, anchor, count), lambda: t.score(logits, anchor, count), B * K),
                 ('add, detections [%d, %d]' % (B, K), lambda: f.add(logits, anchor, count), lambda: t.add_indexed(logits, anchor, count), B * K),
                 ('score_anchors [%d, %d]' % (B, N), lambda: f.score_anchors(logits), lambda: t.rows(logits), B * N),
                 ('add, anchors with max z >= 4 [%d, %d]' % (B, N), lambda: f.add(logits, min_max_logit=thr), lambda: t.add(logits, min_max=thr), B * N))
        for label, new, old, rows in pairs:
            for fn in (new, old):
                window(fn, 2)
            tn, to = [], []
            for _ in range(a.rounds):
                tn.append(window(new, a.iters))
                to.append(window(old, a.iters))
            mn, mo = statistics.median(tn), statistics.median(to)
            rate = rows * C * 2 / (mn * 1e-6)
            say('  %-40s HIP %10.1f us (%10.1f .. %10.1f)   torch %10.1f us (%10.1f .. %10.1f)   ratio torch / HIP %.2f   HIP reads %.3f TB/s, %.2f %% of 8 TB/s'
                % (label, mn, min(tn), max(tn), mo, min(to), max(to), mo / mn, rate / 1e12, 100.0 * rate / PEAK_HBM))
        del f, t, logits
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, 'w') as fo:
            fo.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
