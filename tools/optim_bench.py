#!/usr/bin/env python
"""Time of one optimizer step on the parameter-tensor lists of create_model('tf_efficientdet_d0') (460 tensors, 4.06 M parameters
with its 90 classes) and create_model('tf_efficientdet_d4') (883 tensors, 21.4 M): optim.GroupedOptimizer.step() against
optim.FlatAdam.step() and against torch.optim.Adam(foreach=True) + clip_grad_norm_, one group and one clip domain each, so
that all three do the same work.  A fourth line times the grouping of
infer.py:259-274 / :803-804 (four groups, two clip domains, the backbone / BiFPN / box head only clipped) on the d0 list.

    python3 tools/optim_bench.py [--iters 100] [--rounds 5]

The paths alternate, `--rounds` windows of `--iters` steps each after warm-up (HIP events around a window, host launch overhead
included); the report is the median window and the min .. max spread per path, and the achieved rate on the bytes a step has to
move: 32 B per parameter (read p, g, m, v; write p, m, v; read g once more for the norm).  Needs the GPU: there is no fallback."""
import argparse
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ood_object_detection_amd import optim  # noqa: E402

BYTES_PER_PARAM = 32


def window(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters


def fresh(shapes, dev, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(tuple(s), generator=g).to(dev)) for s in shapes]


def fill_grads(params, seed):
    """small gradients (norm below the clip threshold: torch's clip then leaves them as they are, window after window)"""
    g = torch.Generator().manual_seed(seed)
    for p in params:
        v = (torch.randn(tuple(p.shape), generator=g) * 1e-3).to(p.device)
        if p.grad is None:
            p.grad = v
        else:
            p.grad.copy_(v)


def report(name, t, n_params, a):
    med = statistics.median(t)
    print('%-58s median %8.1f us, spread %8.1f .. %8.1f us  (%d windows of %d)  %.2f TB/s of %d B per parameter'
          % (name, med, min(t), max(t), a.rounds, a.iters, n_params * BYTES_PER_PARAM / (med * 1e-6) / 1e12, BYTES_PER_PARAM))
    return med


def same_work(tag, shapes, dev, a):
    n_params = sum(int(torch.Size(s).numel()) for s in shapes)
    pg, pf, pt = fresh(shapes, dev, 1), fresh(shapes, dev, 1), fresh(shapes, dev, 1)
    grouped = optim.GroupedOptimizer([{'params': pg}], optim='adam', lr=1e-3, clip_domains=[{'params': pg, 'max_norm': 10.0}])
    flat = optim.FlatAdam(pf, lr=1e-3, max_grad_norm=10.0)
    stock = torch.optim.Adam(pt, lr=1e-3, foreach=True)
    for ps in (pg, pf, pt):
        fill_grads(ps, 2)

    def torch_path():
        torch.nn.utils.clip_grad_norm_(pt, 10.0, foreach=True)
        stock.step()
    paths = [('GroupedOptimizer.step()  (3 launches)', grouped.step), ('FlatAdam.step()  (3 launches)', flat.step),
             ('torch.optim.Adam(foreach=True) + clip_grad_norm_', torch_path)]
    print('%s: %d parameter tensors, %.2f M parameters (%.2f M floats with padding in the grouped layout, %d pieces), %.1f MB per step'
          % (tag, len(shapes), n_params / 1e6, grouped.flat_param.numel() / 1e6, grouped.layout['pieces'].shape[0],
             n_params * BYTES_PER_PARAM / 1e6))
    for _ in range(3):
        for _, fn in paths:
            window(fn, 10)
    times = [[] for _ in paths]
    for _ in range(a.rounds):
        for t, (_, fn) in zip(times, paths):
            t.append(window(fn, a.iters))
    med = [report(name, t, n_params, a) for t, (name, _) in zip(times, paths)]
    print('ratio FlatAdam / grouped: %.3f, torch / grouped: %.2f' % (med[1] / med[0], med[2] / med[0]))
    worst = max(float((x.detach() - y.detach()).abs().max()) for x, y in zip(pg, pf))
    print('same outputs: parameters of the grouped and the flat optimizer differ by at most %.2e after all windows' % worst)
    print()


def infer_grouping(model, dev, a):
    """infer.py --train_fpn: predict_pars / class_pars / proj_net / learnable_lr, clips over proj_net and over the whole model"""
    from ood_object_detection_amd.effdet.aux_nets import ProjectionNet
    net = types.SimpleNamespace()
    for part in ('backbone', 'fpn', 'class_net', 'box_net'):
        setattr(net, part, fresh([tuple(p.shape) for p in getattr(model, part).parameters()], dev, 3))
    proj = fresh([tuple(p.shape) for p in ProjectionNet(types.SimpleNamespace(fpn_channels=model.config.fpn_channels), 512).parameters()], dev, 4)
    lrs = [torch.nn.Parameter(torch.tensor(0.01, device=dev)) for _ in range(5)]
    predict, rest = net.class_net[-2:], net.class_net[:-2]
    everything = net.backbone + net.fpn + net.class_net + net.box_net
    groups = [{'params': predict, 'lr': 1e-3}, {'params': rest, 'lr': 1e-3}, {'params': proj, 'lr': 1e-3}, {'params': lrs, 'lr': 0.}]
    domains = [{'params': proj, 'max_norm': 10.0}, {'params': everything, 'max_norm': 10.0}]
    opt = optim.GroupedOptimizer(groups, optim='adam', clip_domains=domains)
    fill_grads(everything + proj + lrs, 5)
    updated = sum(p.numel() for g in groups for p in g['params'])
    normed = sum(p.numel() for d in domains for p in d['params'])
    for _ in range(3):
        window(opt.step, 10)
    t = [window(opt.step, a.iters) for _ in range(a.rounds)]
    med = statistics.median(t)
    moved = updated * 28 + normed * 4
    print('infer.py grouping on the d0 list (4 groups, 2 clip domains): %.2f M parameters updated, %.2f M in the norms, %.1f MB per step'
          % (updated / 1e6, normed / 1e6, moved / 1e6))
    print('%-58s median %8.1f us, spread %8.1f .. %8.1f us  (%d windows of %d)  %.2f TB/s'
          % ('GroupedOptimizer.step()  (3 launches)', med, min(t), max(t), a.rounds, a.iters, moved / (med * 1e-6) / 1e12))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'optim_bench needs the GPU'
    dev = 'cuda:0'
    from ood_object_detection_amd.effdet.factory import create_model
    d0 = None
    for name in ('tf_efficientdet_d0', 'tf_efficientdet_d4'):
        model = create_model(name, pretrained=False, pretrained_backbone=False)
        d0 = d0 or model
        same_work(name, [tuple(p.shape) for p in model.parameters()], dev, a)
    infer_grouping(d0, dev, a)


if __name__ == '__main__':
    main()
