#!/usr/bin/env python
"""One sha256 per call of the episode stage's public API (episode.cluster; projection_losses with its backward; support_loss with its
first and second order gradients) over every tensor the call returns, on seeded inputs, NaNs canonicalised, for an A/B of two
source trees on the same GPU: the file uses nothing but the public API and the test helpers, so a copy of it runs in a checkout of
another commit, and two trees that compute the same bits print the same lines.

    python3 tools/episode_bits.py > bits.txt          a few seconds; needs the GPU

Shapes (num_images, rows, d), each the smallest that reaches one code path; every shape takes its decisions from episode.cluster
itself and covers 'max' / 'avg', the three loss modes, thresh_grad on / off, dot_mult / dot_add / cls_id as numbers and as device
tensors, and one run with an all-false valid set (and one with an all-true set where cluster finds no valid prototype)."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import torch  # noqa: E402

import _episode_loss_ref as lref  # noqa: E402
import _episode_ref as ref  # noqa: E402
from ood_object_detection_amd import episode  # noqa: E402

DEV = 'cuda:0'
SHAPES = [(1, 7, 40),            # m = 1, d below a wave
          (5, 37, 100),          # d not a multiple of 64
          (7, 100, 64),          # n = 700: three parts
          (32, 9, 512),          # d and m d at their limits
          (25, 340, 64),         # n = 8 500: the 32-part cap, and 16 in the second pass
          (64, 260, 64)]         # n = 16 640: the 1 024-block cap, 17 rows per block, m at its limit
DM, DA = 1.5, 0.25


def emit(what, tensors):
    """one line: the digest of the call's tensors in order (shape, dtype and bytes of each; None where nothing flows)"""
    h = hashlib.sha256()
    for t in tensors:
        if t is None:
            h.update(b'none')
            continue
        t = t.detach().cpu().contiguous()
        if t.is_floating_point():
            t = torch.where(torch.isnan(t), torch.full_like(t, float('nan')), t)
        h.update(('%s %s ' % (tuple(t.shape), t.dtype)).encode())
        h.update(t.numpy().tobytes())
    print('%s: %d tensors %s' % (what, len(tensors), h.hexdigest()))


def dots(as_tensors, grad):
    if as_tensors:
        return torch.tensor(DM, device=DEV, requires_grad=grad), torch.tensor(DA, device=DEV, requires_grad=grad)
    return DM, DA


def main():
    assert torch.cuda.is_available(), 'episode_bits needs the GPU'
    for shape_no, (num, rows, d) in enumerate(SHAPES):
        n, seed = num * rows, 10 + shape_no
        x, _ = ref.clustered_rows(seed, num, rows, d)
        gen = torch.Generator().manual_seed(seed)
        confs, logits = torch.randn(n, generator=gen), 2. * torch.randn(n, generator=gen)
        V = [torch.randn(n, d, generator=gen).to(DEV), torch.randn(n, generator=gen).to(DEV), torch.randn(n, generator=gen).to(DEV),
             torch.randn((), generator=gen).to(DEV), torch.randn((), generator=gen).to(DEV)]
        labs = lref.draw_labels(seed, n, True).to(DEV)
        xg, cg, lg = x.to(DEV), confs.to(DEV), logits.to(DEV)
        for sim_target in ('max', 'avg'):
            tag = '%dx%d d%d %s' % (num, rows, d, sim_target)
            sel = episode.cluster(xg, cg, num, DM, DA, None, sim_target)
            emit(tag + ' cluster', [sel[k] for k in sorted(sel)])
            sel_t = episode.cluster(xg, cg, num, *dots(True, False), 0.3, sim_target)
            emit(tag + ' cluster dots on the device, threshold 0.3', [sel_t[k] for k in sorted(sel_t)])
            sels = [('', sel), (' no valid prototype', dict(sel, valid=torch.zeros_like(sel['valid'])))]
            if int(sel['n_valid']) == 0:
                sels.append((' every prototype valid', dict(sel, valid=torch.ones_like(sel['valid']))))
            for sel_name, s in sels:
                for as_tensors in (False, True):
                    where = tag + sel_name + (' on the device' if as_tensors else ' by value')
                    cls = torch.tensor(lref.CLS_ID, device=DEV) if as_tensors else lref.CLS_ID
                    for mode in ('separate', 'same', 'no_conf'):
                        e, c = xg.clone().requires_grad_(), cg.clone().requires_grad_()
                        dm, da = dots(as_tensors, True)
                        o = episode.projection_losses(e, c, labs, cls, s, dm, da, sim_target, mode, 0.1)
                        total = 0.7 * o['clust_loss'] + 0.7 * o['embds_loss'] + 0.01 * o['obj_loss']
                        grads = torch.autograd.grad(total, [e, c] + ([dm, da] if as_tensors else []))
                        emit('%s projection_losses %s' % (where, mode),
                             [o['clust_loss'], o['embds_loss'], o['obj_loss'], o['inner_target'], o['counts']] +
                             [o['stats'][k] for k in episode.STAT_NAMES] + list(grads))
                    for thresh_grad in (True, False):
                        e, c, lo = xg.clone().requires_grad_(), cg.clone().requires_grad_(), lg.clone().requires_grad_()
                        dm, da = dots(as_tensors, True)
                        leaves = [e, c, lo] + ([dm, da] if as_tensors else [])
                        g = torch.tensor(0.8, device=DEV, requires_grad=True)
                        o = episode.support_loss(e, c, lo, s, dm, da, sim_target, thresh_grad)
                        first = torch.autograd.grad(o['loss'], leaves, grad_outputs=g, create_graph=True, allow_unused=True)
                        scalar = sum((gi * v).sum() for gi, v in zip(first, V) if gi is not None)
                        second = torch.autograd.grad(scalar, [g] + leaves, allow_unused=True)
                        emit('%s support_loss thresh_grad=%d' % (where, thresh_grad), [o['loss'], o['target']] + list(first) + list(second))
    torch.cuda.synchronize()


if __name__ == '__main__':
    main()
