#!/usr/bin/env python
"""One sha256 per tensor group of the float32 training path on seeded inputs, NaNs canonicalised, for an A/B of two source trees on the
same GPU (the precedent is tools/episode_bits.py): the file uses nothing but the public API and the test helpers, so a copy of it
runs in a checkout of another commit, and two trees that compute the same bits print the same lines.

    python3 tools/train_param_bits.py > bits.txt          about a minute; needs the GPU

Whole network, tf_efficientdet_d0 at 128 px, 2 images, three steps each (the step that records the stage tables, the first step
that runs them, the steady state) - the loss, every parameter gradient and every BatchNorm buffer after each step (a line
per module group):
    head BatchNorm in batch-statistics mode and in eval mode; bifpn_attn and bifpn_sum besides the default fusion; the 'not_cls'
    stage; one forward + backward of MetaHead's single-node path (first_order).
Then the parameter-sized entry points called directly at the shapes of tests/test_train_param_gpu.py."""
import ctypes
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import _meta_head_cases as mc  # noqa: E402
from _models import seeded_model  # noqa: E402
from _seeded import seeded_array  # noqa: E402
from ood_object_detection_amd import _lib  # noqa: E402
from ood_object_detection_amd.effdet.loss import DetectionLoss  # noqa: E402

DEV = 'cuda:0'
SIZE, B, C = 128, 2, 12


def emit(what, tensors):
    """one line: the digest of the named tensors in order (name, shape, dtype and bytes of each; 'none' where nothing flows)"""
    h = hashlib.sha256()
    for name, t in tensors:
        h.update(name.encode())
        if t is None:
            h.update(b' none')
            continue
        t = t.detach().cpu().contiguous()
        if t.is_floating_point():
            t = torch.where(torch.isnan(t), torch.full_like(t, float('nan')), t)
        h.update((' %s %s ' % (tuple(t.shape), t.dtype)).encode())
        h.update(t.numpy().tobytes())
    print('%s: %d tensors %s' % (what, len(tensors), h.hexdigest()))


def set_bn_eval(m):
    if isinstance(m, torch.nn.BatchNorm2d):
        m.eval()


def targets(cfg, seed):
    rs = np.random.RandomState(seed)
    cls_t, box_t = [], []
    for l in range(cfg.num_levels):
        s = SIZE // (2 ** (cfg.min_level + l))
        cls_t.append(torch.from_numpy(rs.choice([-2, -1, -1, -1, -1, -1, 0, 3, C - 1], size=(B, s, s, 9)).astype(np.int64)).to(DEV))
        t = rs.normal(0, 0.2, (B, s, s, 36)).astype(np.float32)
        t[rs.uniform(size=t.shape) < 0.7] = 0.0
        box_t.append(torch.from_numpy(t).to(DEV))
    return cls_t, box_t, torch.tensor([7.0, 4.0], device=DEV)


def emit_state(tag, model, loss):
    """the loss, then one line per module group (the first two components of the name) and kind: a line per tensor of the ~1 200
    of a step would make the committed outputs larger than the repository allows"""
    torch.cuda.synchronize()
    emit(tag + ' loss', [('loss', loss)])
    groups = {}
    for n, p in model.named_parameters():
        groups.setdefault('grad ' + '.'.join(n.split('.')[:2]), []).append((n, p.grad))
    for n, b in model.named_buffers():
        if 'running_' in n or n.endswith('num_batches_tracked'):
            groups.setdefault('buffer ' + '.'.join(n.split('.')[:2]), []).append((n, b))
    for k in sorted(groups):
        emit('%s %s' % (tag, k), groups[k])


def network(tag, seed, fpn_name=None, head_bn_train=True, not_cls=False):
    model, cfg, _, _ = seeded_model('tf_efficientdet_d0', SIZE, C, seed=seed, fpn_name=fpn_name)
    x = torch.from_numpy(seeded_array(seed, 'input', (B, 3, SIZE, SIZE))).to(DEV)
    model = model.to(DEV).float().train()
    (model if not head_bn_train else model.backbone).apply(set_bn_eval)
    cfg.alpha, cfg.box_loss_weight = 0.15, 50.0
    loss_fn, tg = DetectionLoss(cfg), targets(cfg, seed)
    for step in range(3):
        model.zero_grad(set_to_none=True)
        if not_cls:
            activs, box = model(model(x, mode='bb'), mode='not_cls')
            outs = list(activs) + list(box)
            loss = sum((o * torch.from_numpy(seeded_array(seed, 'w%d' % i, tuple(o.shape))).to(DEV)).sum() for i, o in enumerate(outs))
        else:
            cls_o, box_o = model(x)
            loss = loss_fn(cls_o, box_o, *tg)[0]
        loss.backward()
        emit_state('%s step %d' % (tag, step), model, loss)
    model.autograd = None


def meta_head():
    f, levels = 64, mc.GRAD_LEVELS
    _, _, _, mh = mc.build_meta_head(mc.NAME_OF[f], mc.MAIN_SEED[f])
    mh = mh.to(DEV).float()
    mh.first_order = True
    names, params = [n for n, _ in mh.named_parameters()], list(mh.parameters())
    xs = [t.to(DEV).requires_grad_() for t in mc.level_inputs(mc.MAIN_SEED[f], f, levels)]
    cot = mc.grad_cotangents(f, 9, levels, names, [p.shape for p in params])
    outs, acts, g, _ = mc.first_and_second_order(lambda x_, ret_activs: mh(x_, ret_activs=ret_activs), names, params, xs, cot, second=False)
    torch.cuda.synchronize()
    emit('meta head first_order outputs', [('out%d' % i, t) for i, t in enumerate(outs + acts)])
    for k in sorted(g):
        emit('meta head first_order grad %s' % k, [(k, g[k])])


# ------------------------------------------------------------------------------------------------------------------
# the entry points on their own
# ------------------------------------------------------------------------------------------------------------------
def direct():
    lib = _lib.load()
    st = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
    gen = torch.Generator().manual_seed(99)
    rn = lambda *s: torch.randn(*s, generator=gen).to(DEV)
    pos = lambda *s: (0.25 + torch.rand(*s, generator=gen)).to(DEV)
    new = lambda *s: torch.full(s, float('nan'), dtype=torch.float32, device=DEV)
    P = lambda ts: [None if t is None else t.data_ptr() for t in ts]

    def run(name, tag, outs, *args):
        _lib.check(getattr(lib, name)(st, *args), name)
        torch.cuda.synchronize()
        emit('%s %s' % (name, tag), [('out%d' % i, t) for i, t in enumerate(outs)])

    for N, K in [(1, 1), (24, 27), (40, 240), (300, 257)]:
        W, v = rn(N, K), [rn(N), rn(N), rn(N), pos(N)]
        for wf in (1, 0):
            o = [new(N, K) if wf else None, new(K, N), new(K, N), new(N), new(N), new(N)]
            run('effdet_train_fold_bn', '%dx%d wf%d' % (N, K, wf), o, W.data_ptr(), N, K, *(P(v) + [1e-3] + P(o)))
        ext, sc, rs, mean = rn(N * K + N), rn(N), pos(N), rn(N)
        for tr in (0, 1):
            o = [new(N, K), new(N), new(N)]
            run('effdet_train_convbn_grads', '%dx%d transposed%d' % (N, K, tr), o, ext.data_ptr(), N, K, tr, *(P([W, sc, rs, mean]) + P(o)))
    for n in (2, 3):
        e = rn(n) + 0.5
        for method, src in ((0, e), (1, e), (2, None), (0, -e.abs() - 0.1)):
            o = [new(4)]
            run('effdet_train_fpn_weights', 'n%d method%d%s' % (n, method, '' if src is None or src is e else ' negative'), o,
                None if src is None else src.data_ptr(), n, method, o[0].data_ptr())
    for Cn in (8, 40, 300):
        v = [rn(Cn), pos(Cn), rn(Cn), rn(Cn)]
        for train in (0, 1):
            o = [rn(Cn), pos(Cn), torch.tensor(5, device=DEV), new(Cn), new(Cn), new(Cn)]
            run('effdet_train_bn_finalize', 'C%d train%d' % (Cn, train), o, *(P(v) + P(o[:3]) + [Cn, train, 0.01, 50.0 / 49.0, 1e-3] + P(o[3:])))
    for R, Cn in [(7, 8), (300, 40), (3000, 72)]:
        floats = lib.effdet_train_col_reduce_workspace_floats(1, R, Cn)
        ws = new(floats)
        a, dy = rn(R, Cn) * 1.5 + 0.3, rn(R, Cn)
        mean, rstd = a.double().mean(0).float(), pos(Cn)
        o, gb = [rn(Cn), pos(Cn), torch.tensor(5, device=DEV), new(Cn), new(Cn), new(Cn)], [rn(Cn), rn(Cn)]
        run('effdet_train_bn_var_finalize', '%dx%d' % (R, Cn), o, a.data_ptr(), mean.data_ptr(), R, Cn, *(P(gb) + P(o[:3]) +
            [0.01, R / (R - 1), 1e-3] + P(o[3:]) + [ws.data_ptr(), floats]))
        o = [new(4, Cn)]
        run('effdet_train_bn_bwd_sums', '%dx%d' % (R, Cn), o, *(P([dy, a, mean, rstd]) + [R, Cn, o[0].data_ptr(), ws.data_ptr(), floats]))
        sums, o = new(2, Cn), [new(4, Cn)]
        _lib.check(lib.effdet_train_col_reduce(st, 4, dy.data_ptr(), a.data_ptr(), mean.data_ptr(), 1, R, Cn, sums.data_ptr(), ws.data_ptr(),
                                               floats, 1.0), 'effdet_train_col_reduce')
        run('effdet_train_bn_bwd_prep', '%dx%d' % (R, Cn), o, *(P([sums[0], sums[1], rstd]) + [Cn, 1.0 / R] + P(list(o[0]))))
    for train in ((1,), (0,), (1, 0, 0, 1)):
        for Cn in (8, 72):
            L = len(train)
            vp, cf = ctypes.c_void_p * L, ctypes.c_float * L
            rows = [2 * 3 ** (l + 1) for l in range(L)]
            per = [[rn(Cn), rn(Cn), rn(Cn), pos(Cn), torch.tensor(5, device=DEV)] for _ in range(L)]      # gamma, beta, running stats, nbt
            sums, sq, o = rn(L, Cn) * 4.0, pos(L, Cn) * 9.0, new(4, L, Cn)
            tag = 'L%d C%d train %s' % (L, Cn, ''.join(map(str, train)))
            run('effdet_train_levels_bn_finalize', tag, [o] + [t for p in per for t in p[2:]], sums.data_ptr(), sq.data_ptr(), L, Cn,
                *([vp(*[p[j].data_ptr() for p in per]) for j in range(5)] + [(ctypes.c_int * L)(*train), cf(*[1.0 / r for r in rows]),
                  cf(*[r / (r - 1) for r in rows]), cf(*[0.01 * (l + 1) for l in range(L)]), cf(*[1e-3 * (l + 1) for l in range(L)])] +
                  P(list(o))))
            s2, rstd, o = rn(L, 2, Cn) * 5.0, pos(L, Cn), new(4, L, Cn)
            run('effdet_train_levels_bn_bwd_prep', tag, [o], s2.data_ptr(), rstd.data_ptr(), cf(*[1.0 / r for r in rows]), L, Cn, *P(list(o)))


def main():
    assert torch.cuda.is_available(), 'train_param_bits needs the GPU'
    network('fastattn batch-stats', 27)
    network('fastattn bn-eval', 27, head_bn_train=False)
    network('attn batch-stats', 37, fpn_name='bifpn_attn')
    network('sum batch-stats', 43, fpn_name='bifpn_sum')
    network('not_cls batch-stats', 21, not_cls=True)
    meta_head()
    direct()
    torch.cuda.synchronize()


if __name__ == '__main__':
    main()
