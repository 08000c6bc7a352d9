#!/usr/bin/env python
"""Times of ood_vmf.VMFHead (csrc/vmf.hip) on seeded embeddings against the torch composition on the same GPU.

  sizes     the cells of d0 / 640 (P = 8525, A = 9, K = 76 725 anchors an image) at 8 and at 64 images, C = 90, d in {16, 64}; about
            1.5 % of the anchors carry a seeded label in [0, C).  The embeddings are seeded values; the network does not run.
  train     `head.loss(U, labels)` forward + backward: partition, ordered prototype update, loss, dU and d theta (HIP), and its
            parts (update alone, loss alone).  torch: the loss as `F.normalize`, a matmul, `logsumexp` and autograd over the rows
            picked by `nonzero` (which synchronises; log Z is handed over as a constant from the device table - torch has no Bessel
            function of general order on the GPU, the paper's code leaves the device for it), with the prototype update as (a) the
            paper's per-sample loop and (b) a per-class batched form, mu <- normalize(alpha^n mu + (1 - alpha) sum_i alpha^(n-1-i) r_i),
            which drops the normalisations between the rows and so does not give the loop's numbers.
  one class the update when a single class holds every row: the longest sequential chain a step can have, with and without
            ema_rows_per_class.
  scores    `_score_embeddings` at 100 anchors an image and at every cell, against normalize + matmul + max in torch.

  step      `tools/pretrain_bench.py`'s configuration (tf_efficientdet_d0, 640 px, 8 images, C = 90, float32, labels assigned on the
            GPU, captured iteration) without a head - the code the step ran before the head existed - and with
            `PretrainStep(vmf_head=VMFHead(..., dim=64), vmf_weight=1.5)`, alternated windows of steps in one process.

The paths alternate, `--rounds` windows of calls between two device events (host launch overhead included); the report is the
median window and the min .. max spread per path.

    python3 tools/vmf_bench.py [--out profiles/vmf_bench.txt] [--no-step] [--no-head]     needs the GPU"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from ood_object_detection_amd.ood_vmf import VMFHead, partition, _score_embeddings, update_prototypes  # noqa: E402


def window(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters


def draw(B, P, A, C, d, dev, seed, share=0.015):
    gen = torch.Generator(device=dev).manual_seed(seed)
    dirs = torch.randn(C, d, generator=gen, device=dev)
    cell_cls = torch.randint(0, C, (B, P), generator=gen, device=dev)
    U = (dirs[cell_cls] + 0.35 * d ** 0.5 * torch.randn(B, P, d, generator=gen, device=dev)) * (0.5 + 2.5 * torch.rand(B, P, 1, generator=gen, device=dev))
    pos = torch.rand(B, P, A, generator=gen, device=dev) < share
    labels = torch.where(pos, cell_cls[:, :, None].expand(B, P, A), torch.full((B, P, A), -1, dtype=torch.int64, device=dev)).reshape(B, P * A)
    return U.contiguous(), labels.contiguous()


def torch_rows(U, labels, A, C):
    B, P, d = U.shape
    idx = ((labels >= 0) & (labels < C)).reshape(-1).nonzero().squeeze(1)        # (synchronises)
    return idx // A, labels.reshape(-1)[idx]


def torch_loss(U, labels, A, proto, valid, log_kappa, logz):
    B, P, d = U.shape
    cell, y = torch_rows(U, labels, A, proto.shape[0])
    r = F.normalize(U.reshape(B * P, d)[cell], dim=1, eps=1e-12)
    kappa = log_kappa.clamp(-4.852030263919617, 9.010913347279288).exp()
    l = logz[None] + kappa[None] * (r @ proto.t())
    l = l.masked_fill(~valid[None], float('-inf'))
    return (torch.logsumexp(l, 1) - l.gather(1, y[:, None]).squeeze(1)).mean()


def torch_update_loop(U, labels, A, proto, valid, alpha):
    B, P, d = U.shape
    cell, y = torch_rows(U, labels, A, proto.shape[0])
    r = F.normalize(U.reshape(B * P, d)[cell], dim=1, eps=1e-12)
    for i, c in enumerate(y.tolist()):
        proto[c] = F.normalize(alpha * proto[c] + (1 - alpha) * r[i], dim=0, eps=1e-12)
        valid[c] = True


def torch_update_batched(U, labels, A, proto, valid, alpha):
    B, P, d = U.shape
    C = proto.shape[0]
    cell, y = torch_rows(U, labels, A, C)
    r = F.normalize(U.reshape(B * P, d)[cell], dim=1, eps=1e-12)
    hot = F.one_hot(y, C).to(r.dtype)                                             # [m, C]
    after = hot.flip(0).cumsum(0).flip(0) - hot                                   # rows of the same class that follow
    w = (1 - alpha) * alpha ** (after * hot).sum(1)
    n_c = hot.sum(0)
    v = alpha ** n_c[:, None] * proto + hot.t() @ (w[:, None] * r)
    proto.copy_(torch.where(n_c[:, None] > 0, F.normalize(v, dim=1, eps=1e-12), proto))
    valid |= n_c > 0


def report(say, name, times):
    say('  %-44s %s' % (name, '   '.join('%s %10.1f us (%10.1f .. %10.1f)' % (k, statistics.median(v), min(v), max(v)) for k, v in times.items())))


def bench(a, say, dev):
    C, A, size = 90, 9, 640
    P = sum((size // 2 ** l) ** 2 for l in range(3, 8))
    for B in (8, 64):
        for d in (16, 64):
            U, labels = draw(B, P, A, C, d, dev, 640 + B + d)
            head = VMFHead(64, C, A, dim=d).to(dev)
            leaf = U.clone().requires_grad_()
            m = int(((labels >= 0) & (labels < C)).sum())
            say()
            say('d0 / 640 / %d images, C = %d, d = %d, P = %d, K = %d: %d counted anchors' % (B, C, d, P, A * P, m))

            def train():
                leaf.grad = None
                head.log_kappa.grad = None
                loss, _ = head.loss(leaf, labels)
                loss.backward()

            def upd():
                update_prototypes(U, labels, A, head.prototypes, head.valid, head.ema, None)

            def loss_only():
                leaf.grad = None
                loss, _ = head.loss(leaf, labels, update=False)
                loss.backward()

            train()
            logz = partition(head.log_kappa, d)['logz']
            proto_t, valid_t = torch.zeros(C, d, device=dev), torch.zeros(C, dtype=torch.bool, device=dev)
            torch_update_batched(U, labels, A, proto_t, valid_t, head.ema)

            def lit_loss():
                leaf.grad = None
                torch_loss(leaf, labels, A, proto_t, valid_t, head.log_kappa, logz).backward()

            def lit_batched():
                torch_update_batched(U, labels, A, proto_t, valid_t, head.ema)

            def lit_loop():
                torch_update_loop(U, labels, A, proto_t, valid_t, head.ema)

            l_hip = float(head.loss(leaf, labels, update=False)[0])
            with torch.no_grad():
                proto_t.copy_(head.prototypes)
                valid_t.copy_(head.valid.bool())
            say('  loss %.6f, torch on the same prototypes %.6f' % (l_hip, float(torch_loss(leaf, labels, A, proto_t, valid_t, head.log_kappa, logz))))
            iters = a.iters if B == 8 else max(2, a.iters // 4)
            for fn in (train, upd, loss_only, lit_loss, lit_batched):
                window(fn, 2)
            t = {k: [] for k in ('train', 'update', 'loss', 'torch loss', 'torch batched update')}
            for _ in range(a.rounds):
                t['train'].append(window(train, iters))
                t['update'].append(window(upd, iters))
                t['loss'].append(window(loss_only, iters))
                t['torch loss'].append(window(lit_loss, iters))
                t['torch batched update'].append(window(lit_batched, iters))
            for k in t:
                report(say, k, {'': t[k]})
            if B == 8:
                loop = [window(lit_loop, 1) for _ in range(2)]
                report(say, "torch per-sample update (the paper's loop)", {'': loop})
            # the longest chain: every row in one class
            one = torch.where(labels >= 0, torch.zeros_like(labels), labels)
            for limit in (None, 64):
                def chain():
                    update_prototypes(U, one, A, head.prototypes, head.valid, head.ema, limit)
                window(chain, 2)
                report(say, 'update, one class holds all %d rows, limit %r' % (m, limit), {'': [window(chain, iters) for _ in range(a.rounds)]})
            # scores
            K = 100
            anchor = torch.randint(0, A * P, (B, K), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
            count = torch.full((B,), K, dtype=torch.int32, device=dev)
            kappa = head.log_kappa.detach().exp()

            def lit_cells():
                r = F.normalize(U, dim=2, eps=1e-12)
                dot = (r @ head.prototypes.t()).masked_fill(~valid_t[None, None], float('-inf'))
                l = logz + kappa * dot
                return l.max(2), dot.max(2).values

            def lit_sel():
                r = F.normalize(torch.gather(U, 1, (anchor // A)[:, :, None].expand(B, K, d)), dim=2, eps=1e-12)
                dot = (r @ head.prototypes.t()).masked_fill(~valid_t[None, None], float('-inf'))
                l = logz + kappa * dot
                return l.max(2), dot.max(2).values

            hip_cells = lambda: _score_embeddings(head, U)
            hip_sel = lambda: _score_embeddings(head, U, anchor, count)
            for fn in (hip_cells, hip_sel, lit_cells, lit_sel):
                window(fn, 2)
            t = {k: [] for k in ('score, 100 anchors an image', 'torch score', 'score_cells', 'torch score_cells')}
            for _ in range(a.rounds):
                t['score, 100 anchors an image'].append(window(hip_sel, iters))
                t['torch score'].append(window(lit_sel, iters))
                t['score_cells'].append(window(hip_cells, iters))
                t['torch score_cells'].append(window(lit_cells, iters))
            for k in t:
                report(say, k, {'': t[k]})
            del U, labels, leaf, head
            torch.cuda.empty_cache()


def bench_step(a, say, dev):
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    from bench import build_model
    from pretrain_bench import synthetic_targets
    from ood_object_detection_amd.pretrain import PretrainStep
    B, size, C = 8, 640, 90
    x = torch.randint(0, 256, (B, 3, size, size), dtype=torch.uint8, device=dev, generator=torch.Generator(device=dev).manual_seed(100))
    target = synthetic_targets(B, size, C, 7, dev)
    steps = {}
    for name in ('without', 'with'):
        model = build_model('tf_efficientdet_d0', size, C).to(dev).float()
        with torch.no_grad():
            model.class_net.predict.conv_pw.bias.fill_(-4.59511985)
        head = VMFHead(model.config.fpn_channels, C, model.class_net.predict.conv_pw.weight.shape[0] // C, dim=64).to(dev) if name == 'with' else None
        steps[name] = PretrainStep(model, graph=True, vmf_head=head, vmf_weight=1.5)
        for _ in range(4):
            out = steps[name](x, target)
        torch.cuda.synchronize()
        say('  %s the head: loss after 4 steps %.4f%s' % (name, float(out['loss']), '' if head is None else ', vmf_loss %.4f, m %d, valid classes %d' % (
            float(out['vmf_loss']), int(out['vmf_m']), int(out['vmf_valid_classes']))))
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=12)
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--no-step', action='store_true')
    ap.add_argument('--no-head', action='store_true')
    ap.add_argument('--out', default=None, help='also write the report to this file')
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'vmf_bench needs the GPU'
    dev = torch.device('cuda:0')
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)
        if a.out:
            with open(a.out, 'w') as fo:
                fo.write('\n'.join(lines) + '\n')

    say('VMFHead on %s: median microseconds per call of %d alternated windows (min .. max)' % (torch.cuda.get_device_name(0), a.rounds))
    if not a.no_head:
        bench(a, say, dev)
    if not a.no_step:
        say()
        say('pretrain step, tf_efficientdet_d0 / 640 / 8 images / C = 90 / float32, captured iteration, %d windows of %d steps, alternated' % (a.rounds, a.steps))
        bench_step(a, say, dev)


if __name__ == '__main__':
    main()
