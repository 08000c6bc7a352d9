#!/usr/bin/env python
"""Times of ood_synth.OutlierSynthesizer.sample (csrc/outlier_synth.hip) against the literal torch composition on the same GPU, and the
pretrain step with and without the synthesiser.

  sample   C = 90 classes, S = 10 000 candidates, k = 1 and 16, for each BiFPN width F of `ood_features.WIDTHS` (64 .. 288), a random
           well-conditioned tied factor.  torch: per class `MultivariateNormal(mu_c, scale_tril=L).rsample((S,))`, `log_prob`, and
           `topk` of the k smallest - 90 loops that materialise S x F normals each; no host synchronisation on either side.  The paths
           alternate, `--rounds` windows of calls between two device events (host launch overhead included); the report is the median
           window and the min .. max spread per path, and the ratio.  `graph` is the HIP call replayed from a captured graph.
  step     `tools/pretrain_bench.py`'s configuration (tf_efficientdet_d0, 640 px, 8 images, C = 90, float32, labels assigned on the GPU,
           captured iteration) with the logistic regulariser alone - the code of the parent commit - and with the synthesiser (statistics
           added every step, virtual outliers in the loss; the refits are switched off for the timed windows), alternated windows of
           steps in one process.

    python3 tools/outlier_synth_bench.py [--out profiles/outlier_synth_bench.txt] [--no-step]     needs the GPU"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ood_object_detection_amd.ood_features import WIDTHS  # noqa: E402
from ood_object_detection_amd.ood_synth import OutlierSynthesizer  # noqa: E402
from ood_object_detection_amd.ood_train import EnergyRegularizer  # noqa: E402


def window(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters


def gaussians(F, C, seed):
    g = np.random.default_rng(seed)
    mu = g.standard_normal((C, F))
    L = np.tril(g.standard_normal((F, F)) / np.sqrt(F), -1) + np.diag(g.uniform(0.5, 1.5, F))
    return mu, L


def torch_sample(mu, L, S, k):
    rows = []
    for c in range(mu.shape[0]):
        d = torch.distributions.MultivariateNormal(mu[c], scale_tril=L)
        x = d.rsample((S,))
        lp = d.log_prob(x)
        rows.append(x[torch.topk(lp, k, largest=False).indices])
    return torch.stack(rows)


def bench_sample(a, say, dev):
    C, S = 90, 10000
    for F in WIDTHS:
        mu, L = gaussians(F, C, F)
        mu_t, L_t = torch.from_numpy(mu).float().to(dev), torch.from_numpy(L).float().to(dev)
        for k in (1, 16):
            synth = OutlierSynthesizer(F, C, 9, candidates=S, keep=k, seed=1, device=dev).set_gaussians(mu, L)
            hip = lambda: synth.sample()
            lit = lambda: torch_sample(mu_t, L_t, S, k)
            out = hip()
            ref = lit()
            torch.cuda.synchronize()
            note = 'mean r2 of the kept rows %.1f; torch: mean Mahalanobis distance of its kept rows %.1f (chi^2_%d: mean %d)' % (
                float(out['r2'].mean()), float((torch.linalg.solve_triangular(L_t, (ref - mu_t[:, None]).transpose(1, 2), upper=False) ** 2).sum(1).mean()), F, F)
            side = torch.cuda.Stream(dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            g = torch.cuda.CUDAGraph()
            with torch.cuda.stream(side):
                with torch.cuda.graph(g, stream=side):
                    synth.sample()
            torch.cuda.current_stream(dev).wait_stream(side)
            for fn in (hip, lit, g.replay):
                window(fn, 2)
            th, tt, tg = [], [], []
            for _ in range(a.rounds):
                th.append(window(hip, a.iters))
                tt.append(window(lit, max(1, a.iters // 4)))
                tg.append(window(g.replay, a.iters))
            mh, mt, mg = statistics.median(th), statistics.median(tt), statistics.median(tg)
            say('  F %3d k %2d  HIP %8.1f us (%8.1f .. %8.1f)  graph %8.1f us (%8.1f .. %8.1f)  torch %10.1f us (%10.1f .. %10.1f)  ratio %6.1f'
                % (F, k, mh, min(th), max(th), mg, min(tg), max(tg), mt, min(tt), max(tt), mt / mh))
            say('      ' + note)
            del synth, g
        torch.cuda.empty_cache()


def bench_step(a, say, dev):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    from bench import build_model
    from pretrain_bench import synthetic_targets
    from ood_object_detection_amd.pretrain import PretrainStep
    B, size, C = 8, 640, 90
    x = torch.randint(0, 256, (B, 3, size, size), dtype=torch.uint8, device=dev, generator=torch.Generator(device=dev).manual_seed(100))
    target = synthetic_targets(B, size, C, 7, dev)
    target['outlier'] = torch.zeros(B, dtype=torch.bool, device=dev)
    steps = {}
    for name in ('without', 'with'):
        model = build_model('tf_efficientdet_d0', size, C).to(dev).float()
        with torch.no_grad():
            model.class_net.predict.conv_pw.bias.fill_(-4.59511985)
        reg = EnergyRegularizer(C, 'logistic', weight_in=0.1, weight_out=0.1).to(dev)
        synth = OutlierSynthesizer(model.config.fpn_channels, C, 9, candidates=10000, keep=1, seed=1, device=dev) if name == 'with' else None
        kw = {} if synth is None else dict(outlier_synthesizer=synth, synth_refresh_every=2, synth_shrinkage=0.1)
        steps[name] = PretrainStep(model, graph=True, ood_regularizer=reg, **kw)
        for _ in range(6):
            out = steps[name](x, target)
        steps[name].synth_refresh_every = 1 << 40              # no refit (a host read and a Cholesky factorisation) in the timed windows
        torch.cuda.synchronize()
        assert steps[name]._cap is not None
        say('  %s the synthesiser: loss after 6 steps %.4f, ood_loss %.4f, n_in %d%s' % (
            name, float(out['loss']), float(out['ood_loss']), int(out['n_in']),
            '' if synth is None else ', n_virtual %d, rows in the statistics %d' % (int(out['n_virtual']), int(synth.statistics.n_c.sum()))))
    times = {k: [] for k in steps}
    for _ in range(a.rounds):
        for name, step in steps.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step(x, target)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / a.steps)
    mw, mr = statistics.median(times['without']), statistics.median(times['with'])
    say('  step without %.2f ms (%.2f .. %.2f), with %.2f ms (%.2f .. %.2f): + %.2f ms, %.2f %%' % (
        mw, min(times['without']), max(times['without']), mr, min(times['with']), max(times['with']), mr - mw, 100 * (mr - mw) / mw))
    t0 = time.perf_counter()
    steps['with'].synth.fit(0.1)
    torch.cuda.synchronize()
    say('  one refit (host read, float64 Cholesky, four in-place copies): %.2f ms' % ((time.perf_counter() - t0) * 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=12)
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--no-step', action='store_true')
    ap.add_argument('--no-sample', action='store_true')
    ap.add_argument('--out', default=None, help='also write the report to this file')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'outlier_synth_bench needs the GPU'
    dev = torch.device('cuda:0')
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, 'w') as fo:
                fo.write('\n'.join(lines) + '\n')

    say('OutlierSynthesizer.sample on %s: median microseconds per call of %d alternated windows (min .. max), C = 90, S = 10 000'
        % (torch.cuda.get_device_name(0), a.rounds))
    if not a.no_sample:
        bench_sample(a, say, dev)
    if not a.no_step:
        say()
        say('pretrain step, tf_efficientdet_d0 / 640 / 8 images / C = 90 / float32, captured iteration, logistic regulariser, %d windows of %d steps, alternated'
            % (a.rounds, a.steps))
        bench_step(a, say, dev)


if __name__ == '__main__':
    main()
