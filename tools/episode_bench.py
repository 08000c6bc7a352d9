#!/usr/bin/env python
"""Time of the episode stage (anchor selection + ProjectionNet feed + clustering, ood_object_detection_amd/episode.py) against the
literal torch composition of infer.py:362-447 / :566-654 (tests/_episode_ref.py, torch's own kernels on the same GPU).  The
ProjectionNet itself is common to both and left out: both sides cluster the same embeddings.

    python3 tools/episode_bench.py                    meta-phase default (25 images, P5-P7 of 256 px: 756 anchors -> 252 rows, F 160, d 256)
    python3 tools/episode_bench.py --phase proj       projection-phase default (P3-P7: 12 276 anchors -> 1 692 rows per image, 42 300 rows)

The two paths alternate, `--rounds` windows of `--iters` iterations each (HIP events around a window, host launch overhead
included); the report is the median window and the min .. max spread per path.  Needs the GPU: there is no fallback.

    python3 tools/episode_bench.py --losses           episode.projection_losses forward + backward (infer.py:448-498, 787-789) against
                                                      the literal n x n composition with autograd (tests/_episode_loss_ref.py), at the
                                                      meta-phase size (25 x 252 rows) and the projection-phase size (25 x 1 692), d 256
    python3 tools/episode_bench.py --support          episode.support_loss (infer.py:645-658) against target_from_selection +
                                                      F.binary_cross_entropy_with_logits on the same decisions, at the meta-phase default
                                                      (25 x 252 rows, d 256): the loss, the create_graph=True gradient to the embeddings
                                                      and logits, and the backward of a scalar of that gradient
    python3 tools/episode_bench.py --inner            episode.inner_update (infer.py:660-678) forward + backward against the literal
                                                      loop `par - par_lr * inner_grad` with GPU step sizes and autograd, on the d0 head's
                                                      parameter list (F 64, 3 layers, 9 anchors) and the d3 default's (F 160, 4 layers)"""
import argparse
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import _episode_loss_ref as lref  # noqa: E402
import _episode_ref as ref  # noqa: E402
import _inner_update_ref as iref  # noqa: E402
from ood_object_detection_amd import episode  # noqa: E402
from ood_object_detection_amd.effdet.aux_nets import ProjectionNet  # noqa: E402

A = 9


def window(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters


def losses_section(a, dev):
    """projection_losses forward + backward against the literal composition, same decisions, same upstream weights"""
    B, d = a.images, a.width // 2
    for rows in (252, 1692):
        n = B * rows
        x, _ = ref.clustered_rows(2, B, rows, d)
        confs = torch.randn(n, generator=torch.Generator().manual_seed(2))
        labs = lref.draw_labels(2, n, True).to(dev)
        e, c = x.to(dev).requires_grad_(), confs.to(dev).requires_grad_()
        dm, da = torch.tensor(1.5, device=dev, requires_grad=True), torch.tensor(0.25, device=dev, requires_grad=True)
        with torch.no_grad():
            sel = episode.cluster(e, c, B, dm, da)
        leaves = [e, c, dm, da]

        def step(fn):
            o = fn(e, c, labs, lref.CLS_ID, sel, dm, da, 'max', 'separate', 0.)
            return o, torch.autograd.grad(0.03 * (30. * (o['embds_loss'] + o['clust_loss']) + 1e-4 * o['obj_loss']), leaves)

        new_path = lambda: step(episode.projection_losses)
        literal_path = lambda: step(lref.losses_literal)
        print('losses, %d images x %d rows, n = %d, d %d; one n x n float32 matrix is %.1f MB' % (B, rows, n, d, n * n * 4 / 1e6))
        o_new, g_new = new_path()
        literal, iters_lit = not a.no_literal, a.iters if n * n < 1e8 else max(1, a.iters // 20)
        if literal:
            try:
                o_lit, g_lit = literal_path()
                torch.cuda.synchronize()
                print('same outputs: losses differ by %.2e (relative), gradients by %.2e of the largest entry'
                      % (max(float((o_new[k] - o_lit[k]).abs() / o_lit[k].abs().clamp(min=1e-30)) for k in ('clust_loss', 'embds_loss', 'obj_loss')),
                         max(float((p - q).abs().max() / q.abs().max()) for p, q in zip(g_new, g_lit))))
                del o_lit, g_lit
            except torch.OutOfMemoryError:
                print('literal form: cannot run at this size (out of memory with %.0f GB free)' % (torch.cuda.mem_get_info()[0] / 1e9))
                literal = False
            torch.cuda.empty_cache()
        for _ in range(3):
            window(new_path, 5)
            if literal:
                window(literal_path, 2)
        t_new, t_lit = [], []
        for _ in range(a.rounds):
            t_new.append(window(new_path, a.iters))
            if literal:
                t_lit.append(window(literal_path, iters_lit))
        print('projection_losses forward + backward (6 HIP launches): median %.1f us, spread %.1f .. %.1f us  (%d windows of %d)'
              % (statistics.median(t_new), min(t_new), max(t_new), a.rounds, a.iters))
        if literal:
            print('literal torch composition with autograd:               median %.1f us, spread %.1f .. %.1f us  (windows of %d)'
                  % (statistics.median(t_lit), min(t_lit), max(t_lit), iters_lit))
            print('ratio literal / new: %.2f' % (statistics.median(t_lit) / statistics.median(t_new)))
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        new_path()
        torch.cuda.synchronize()
        print('peak memory of one forward + backward: %.1f MB above the %.1f MB of inputs'
              % ((torch.cuda.max_memory_allocated() - base) / 1e6, (e.numel() * 4 + c.numel() * 4 + labs.numel() * 8) / 1e6))
        print()


def support_section(a, dev):
    """support_loss against target_from_selection + BCE: the same decisions, one head (the class logits are the confidences)"""
    B, d, rows = a.images, a.width // 2, 252
    n = B * rows
    x, _ = ref.clustered_rows(2, B, rows, d)
    gen = torch.Generator().manual_seed(2)
    e, c = x.to(dev).requires_grad_(), torch.randn(n, generator=gen).to(dev).requires_grad_()
    dm, da = torch.tensor(1.5, device=dev, requires_grad=True), torch.tensor(0.25, device=dev, requires_grad=True)
    w_e, w_c = torch.randn(n, d, generator=gen).to(dev), torch.randn(n, generator=gen).to(dev)
    with torch.no_grad():
        sel = episode.cluster(e, c, B, dm, da)

    def hip_loss():
        return episode.support_loss(e, c, c, sel, dm, da)['loss']

    def torch_loss():
        return F.binary_cross_entropy_with_logits(c, episode.target_from_selection(e, c, sel, dm, da)['target'])

    def inner(loss_fn):
        return torch.autograd.grad(loss_fn(), [e, c], create_graph=True)

    def outer(loss_fn):
        g = inner(loss_fn)
        return torch.autograd.grad((g[0] * w_e).sum() + (g[1] * w_c).sum(), [e, c, dm, da])

    print('support loss, %d images x %d rows, n = %d, d %d' % (B, rows, n, d))
    with torch.no_grad():
        l_new, l_old = hip_loss(), torch_loss()
    g_new, g_old, h_new, h_old = inner(hip_loss), inner(torch_loss), outer(hip_loss), outer(torch_loss)
    torch.cuda.synchronize()
    print('same outputs: loss differs by %.2e (relative), gradients by %.2e, second-order results by %.2e of the largest entry'
          % (float((l_new - l_old).abs() / l_old.abs()), max(float((p - q).abs().max() / q.abs().max()) for p, q in zip(g_new, g_old)),
             max(float((p - q).abs().max() / q.abs().max()) for p, q in zip(h_new, h_old))))
    del g_new, g_old, h_new, h_old
    stages = [('loss', lambda f: f(), 3), ('loss + create_graph gradient', inner, 6), ('loss + gradient + backward through it', outer, 10)]
    for name, stage, launches in stages:
        paths = [lambda: stage(hip_loss), lambda: stage(torch_loss)]
        if name == 'loss':
            paths = [torch.no_grad()(p) for p in paths]
        for _ in range(3):
            for p in paths:
                window(p, 5)
        t_new, t_old = [], []
        for _ in range(a.rounds):
            t_new.append(window(paths[0], a.iters))
            t_old.append(window(paths[1], a.iters))
        print('%s' % name)
        print('  support_loss (%2d HIP launches):          median %.1f us, spread %.1f .. %.1f us  (%d windows of %d)'
              % (launches, statistics.median(t_new), min(t_new), max(t_new), a.rounds, a.iters))
        print('  target_from_selection + BCE (torch):     median %.1f us, spread %.1f .. %.1f us'
              % (statistics.median(t_old), min(t_old), max(t_old)))
        print('  ratio torch / support_loss: %.2f' % (statistics.median(t_old) / statistics.median(t_new)))


def inner_section(a, dev):
    """inner_update forward + backward against the literal loop: the same tensors, step sizes and cotangents; the gradients go to
    the parameters, to inner_grad (leaves here, standing for the create_graph=True gradient) and to the step sizes"""
    for label, Fc, layers in (('d0 head', 64, 3), ('d3 default', 160, 4)):
        named_shapes = iref.meta_head_shapes(Fc, layers, 5, A)
        names = [n for n, _ in named_shapes]
        cpu = iref.seeded_list(layers, named_shapes)
        ps, gs = ([t.to(dev).requires_grad_() for t in lst] for lst in cpu[:2])
        Ws = [t.to(dev) for t in cpu[2]]
        lrs = [torch.nn.Parameter(torch.tensor(0.05 + 0.02 * k, device=dev)) for k in range(layers + 2)]
        plan = episode.plan_inner_update(names, len(lrs))
        act = [i for i, k in enumerate(plan) if k is not None]
        leaves = [ps[i] for i in act] + [gs[i] for i in act] + lrs
        shared = len(act) - len(set(plan[i] for i in act))

        def step(update):
            fast = update(list(zip(names, ps)), gs, lrs)
            return fast, torch.autograd.grad([fast[i] for i in act], leaves, grad_outputs=[Ws[i] for i in act])

        new_path = lambda: step(episode.inner_update)
        literal_path = lambda: step(iref.literal_update)
        f_new, g_new = new_path()
        f_lit, g_lit = literal_path()
        torch.cuda.synchronize()
        n_t = len(act)
        print('inner update, %s: F %d, %d layers, %d anchors; %d of %d tensors updated, %d elements, %d step sizes'
              % (label, Fc, layers, A, n_t, len(names), sum(ps[i].numel() for i in act), len(lrs)))
        print('same outputs: fast weights bit-equal %s, d inner_grad bit-equal %s, d lr differs by %.2e of the largest entry'
              % (all(torch.equal(p, q) for p, q in zip(f_new, f_lit)), all(torch.equal(p, q) for p, q in zip(g_new[n_t:2 * n_t], g_lit[n_t:2 * n_t])),
                 float((torch.stack(g_new[2 * n_t:]) - torch.stack(g_lit[2 * n_t:])).abs().max() / torch.stack(g_lit[2 * n_t:]).abs().max())))
        del f_new, g_new, f_lit, g_lit
        for _ in range(3):
            window(new_path, 5)
            window(literal_path, 5)
        t_new, t_lit = [], []
        for _ in range(a.rounds):
            t_new.append(window(new_path, a.iters))
            t_lit.append(window(literal_path, a.iters))
        # launches counted from the expressions: mul + sub per tensor forward; neg, grad * lr, grad * g and its sum per tensor
        # backward, plus one add per tensor that shares its step size with an earlier one
        print('inner_update forward + backward (1 + 2 = 3 HIP launches):   median %.1f us, spread %.1f .. %.1f us  (%d windows of %d)'
              % (statistics.median(t_new), min(t_new), max(t_new), a.rounds, a.iters))
        print('literal torch loop with autograd (%d + %d = %d launches):  median %.1f us, spread %.1f .. %.1f us'
              % (2 * n_t, 4 * n_t + shared, 6 * n_t + shared, statistics.median(t_lit), min(t_lit), max(t_lit)))
        print('ratio literal / new: %.2f' % (statistics.median(t_lit) / statistics.median(t_new)))
        print()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--losses', action='store_true', help='time projection_losses forward + backward instead of the episode stage')
    ap.add_argument('--support', action='store_true', help='time support_loss at its three orders instead of the episode stage')
    ap.add_argument('--inner', action='store_true', help='time inner_update forward + backward against the literal torch loop')
    ap.add_argument('--phase', choices=['meta', 'proj'], default='meta')
    ap.add_argument('--images', type=int, default=25)
    ap.add_argument('--fpn', type=int, default=160)
    ap.add_argument('--width', type=int, default=512)
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--no-literal', action='store_true', help='time the new path alone')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'episode_bench needs the GPU'
    dev = 'cuda:0'
    if a.losses:
        return losses_section(a, dev)
    if a.support:
        return support_section(a, dev)
    if a.inner:
        return inner_section(a, dev)
    sides, first = ([8, 4, 2], 2) if a.phase == 'meta' else ([32, 16, 8, 4, 2], 0)
    B, Fc, d = a.images, a.fpn, a.width // 2
    torch.manual_seed(0)
    net = ProjectionNet(types.SimpleNamespace(fpn_channels=Fc), a.width).to(dev)
    gen = torch.Generator().manual_seed(1)
    activs = [torch.randn(B, s, s, Fc, generator=gen).to(dev).permute(0, 3, 1, 2) for s in sides]
    confs = [(ref.tie_free_confs(s, B, A * s * s) - 1.0).to(dev).view(B, s, s, A).permute(0, 3, 1, 2) for s in sides]
    rows = sum(episode.kept_per_level(s, s) for s in sides)
    n = B * rows
    x, _ = ref.clustered_rows(2, B, rows, d)
    embds = x.to(dev)
    thr = 0.3 if a.phase == 'meta' else None

    def new_path():
        sel = episode.select_anchors(confs)
        feed, conf = episode.projection_feed(activs, confs, sel, net, first_level=first)
        return feed, episode.cluster(embds, conf.reshape(-1), B, 3., 3., valid_threshold=thr)

    def literal_path():
        feed, conf, _ = ref.episode_feed(activs, confs, net.anch_enc, net.lev_enc, net.cell_enc, first)
        return feed, ref.cluster_literal(embds, conf.reshape(-1), 3., 3., B, thr, 'max')

    print('%s phase: %d images x %d anchors -> %d rows each, n = %d, F %d, d %d; one n x n float32 matrix is %.1f MB'
          % (a.phase, B, sum(A * s * s for s in sides), rows, n, Fc, d, n * n * 4 / 1e6))
    free = torch.cuda.mem_get_info()[0]
    literal = not a.no_literal
    if literal and 8 * n * n * 4 > free:
        print('literal form: not run (its n x n temporaries do not fit the %.0f GB free)' % (free / 1e9))
        literal = False
    with torch.no_grad():
        f_new, o_new = new_path()
        if literal:
            f_lit, o_lit = literal_path()
            torch.cuda.synchronize()
            agree = o_new['nearest'] == o_lit['nearest']             # near-tied prototypes may be named differently in float32
            print('same outputs: feed bit-equal %s, prototypes equal %s, nearest prototype differs on %d of %d rows, target max diff '
                  'on the others %.2e'
                  % (torch.equal(f_new, f_lit), torch.equal(o_new['proto'], o_lit['proto']), int((~agree).sum()), n,
                     float(((o_new['target'] - o_lit['target']) * agree).abs().max())))
            del f_lit, o_lit
        for _ in range(3):
            window(new_path, 5)
            if literal:
                window(literal_path, 5)
        t_new, t_lit = [], []
        for _ in range(a.rounds):
            t_new.append(window(new_path, a.iters))
            if literal:
                t_lit.append(window(literal_path, a.iters))
    print('new path  (select + feed + cluster, 9 HIP launches): median %.1f us, spread %.1f .. %.1f us  (%d windows of %d)'
          % (statistics.median(t_new), min(t_new), max(t_new), a.rounds, a.iters))
    if literal:
        print('literal torch composition:                           median %.1f us, spread %.1f .. %.1f us'
              % (statistics.median(t_lit), min(t_lit), max(t_lit)))
        print('ratio literal / new: %.2f' % (statistics.median(t_lit) / statistics.median(t_new)))


if __name__ == '__main__':
    main()
