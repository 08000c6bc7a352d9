#!/usr/bin/env python
"""Time of ood.OODEvaluator.evaluate (radix sort of both sides + metrics, csrc/ood_eval.hip; the result block is read back, so
every call ends in a synchronisation) at P = N = 2^16, 2^20 and 2^22 against

  (a) the literal torch composition on the same GPU: torch.sort, torch.searchsorted, cumsum / sums in float64, with the same
      one read-back of the results;
  (b) ood.auroc, the exhaustive pair count (AUROC only), at 2^16 alone - 2^20 x 2^20 pairs do not finish in reasonable time.

The paths alternate, `--rounds` windows of `--iters` calls each between two device events; the report is the median window and
the min .. max spread per path.  Needs the GPU: there is no fallback.

    python3 tools/ood_eval_bench.py [--out profiles/ood_eval_bench.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ood_object_detection_amd import ood  # noqa: E402


def window(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters


def torch_metrics(pos, neg, level):
    """The definitions of OODEvaluator.evaluate in torch ops; float64 wherever a ratio or a sum is formed"""
    P, N = pos.numel(), neg.numel()
    ps, ns = torch.sort(pos)[0], torch.sort(neg)[0]
    lb, ub = torch.searchsorted(ns, ps), torch.searchsorted(ns, ps, right=True)
    gt, eq = lb.sum(), (ub - lb).sum()
    idx = torch.arange(P, device=pos.device)
    end = torch.ones(P, dtype=torch.bool, device=pos.device)
    end[:-1] = ps[1:] != ps[:-1]
    first = torch.searchsorted(ps, ps)
    w = (idx + 1 - first).double() / P
    tp, fp = (P - first).double(), (N - lb).double()
    aupr_in = torch.where(end, w * (tp / (tp + fp)), torch.zeros_like(w)).cumsum(0)[-1]
    jdx = torch.arange(N, device=pos.device)
    endn = torch.ones(N, dtype=torch.bool, device=pos.device)
    endn[:-1] = ns[1:] != ns[:-1]
    firstn = torch.searchsorted(ns, ns)
    wn = (jdx + 1 - firstn).double() / N
    le_n, le_p = (jdx + 1).double(), torch.searchsorted(ps, ns, right=True).double()
    aupr_out = torch.where(endn, wn * (le_n / (le_n + le_p)), torch.zeros_like(wn)).cumsum(0)[-1]
    k = max(1, min(P, int(-(-level * P // 1))))
    thr = ps[P - k]
    tpk = P - torch.searchsorted(ps, thr)
    fpk = N - torch.searchsorted(ns, thr)
    out = torch.stack([gt.double(), eq.double(), aupr_in, aupr_out, tpk.double(), fpk.double(), thr.double()]).tolist()
    return {'auroc': (out[0] + 0.5 * out[1]) / (P * N), 'aupr_in': out[2], 'aupr_out': out[3], 'fpr_at_tpr': out[5] / N, 'tpr': out[4] / P}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[1 << 16, 1 << 20, 1 << 22])
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--level', type=float, default=0.95)
    ap.add_argument('--out', default=None, help='also write the report to this file')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'ood_eval_bench needs the GPU'
    dev = 'cuda:0'
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    say('OODEvaluator.evaluate on %s; scores: in-distribution N(0.4, 1), OOD N(0, 1), float32, P = N' % torch.cuda.get_device_name(0))
    for n in a.sizes:
        gen = torch.Generator(device=dev).manual_seed(n)
        pos = torch.randn(n, generator=gen, device=dev) + 0.4
        neg = torch.randn(n, generator=gen, device=dev)
        ev = ood.OODEvaluator(n, n, dev)
        ev.add(pos, False)
        ev.add(neg, True)
        new_path = lambda: ev.evaluate(a.level)
        lit_path = lambda: torch_metrics(pos, neg, a.level)
        paths = [('evaluate (12 sort + 2 metric launches)', new_path), ('torch.sort + searchsorted + cumsum, float64', lit_path)]
        if n <= 1 << 16:
            paths.append(('ood.auroc pair count (AUROC only)', lambda: ood.auroc(pos, neg)))
        got, lit = new_path(), lit_path()
        say()
        say('P = N = %d (2^%d): auroc %.6f, aupr_in %.6f, aupr_out %.6f, fpr at %.2f tpr %.6f' % (n, n.bit_length() - 1, got['auroc'], got['aupr_in'], got['aupr_out'], a.level, got['fpr_at_tpr']))
        say('  largest difference to the torch composition over auroc, aupr_in, aupr_out, fpr, tpr: %.2e'
            % max(abs(got[k] - lit[k]) for k in lit))
        iters = max(30, min(200, (1 << 25) // n))                       # windows of tens of milliseconds at every size
        for _, p in paths:
            for _ in range(2):
                window(p, max(1, iters // 4))
        times = [[] for _ in paths]
        for _ in range(a.rounds):
            for t, (_, p) in zip(times, paths):
                t.append(window(p, iters))
        for t, (name, _) in zip(times, paths):
            say('  %-46s median %9.1f us, spread %9.1f .. %9.1f us  (%d windows of %d)' % (name, statistics.median(t), min(t), max(t), a.rounds, iters))
        say('  ratio torch composition / evaluate: %.2f' % (statistics.median(times[1]) / statistics.median(times[0])))
        if len(paths) > 2:
            say('  ratio pair count / evaluate: %.2f' % (statistics.median(times[2]) / statistics.median(times[0])))
        t_add = []
        for _ in range(a.rounds):
            ev.clear()
            t_add.append(window(lambda: (ev.clear(), ev.add(pos, False), ev.add(neg, True)), max(1, iters // 4)))
        say('  clear + add of both sides (6 launches):         median %9.1f us, spread %9.1f .. %9.1f us' % (statistics.median(t_add), min(t_add), max(t_add)))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
