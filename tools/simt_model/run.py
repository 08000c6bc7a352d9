#!/usr/bin/env python
"""episode.support_loss's kernels without a GPU: csrc/episode_support.hip compiled by g++ against the CPU model of common.h and
driven through the C ABI on CPU tensors, at all three orders, against the float64 lean form of tests/_support_loss_ref.py - the
comparison of tests/test_support_loss_gpu.py at its small shapes, with the same bounds (values 2e-5, gradients 1e-4, second order
4 E32 + 1e-7 of the largest entry).  Prints one line per configuration and the largest figures; exits 1 on a miss.

    python3 tools/simt_model/run.py            needs g++ with C++20 (std::barrier); a minute or so, a thread per lane"""
import ctypes
import itertools
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import torch  # noqa: E402

import _support_loss_ref as sref  # noqa: E402
from ood_object_detection_amd import _lib  # noqa: E402

SHAPES = [(1, 7, 40, 1), (3, 50, 200, 2), (5, 60, 64, 6)]        # num, rows, d, seed


def build(tmp):
    csrc = os.path.join(ROOT, 'ood_object_detection_amd', 'csrc')
    shutil.copy(os.path.join(HERE, 'common.h'), tmp)
    shutil.copy(os.path.join(csrc, 'episode_rows.h'), tmp)
    shutil.copy(os.path.join(csrc, 'episode_support.hip'), os.path.join(tmp, 'episode_support.cpp'))
    out = os.path.join(tmp, 'libsupport_model.so')
    subprocess.run(['g++', '-std=c++20', '-O1', '-fPIC', '-shared', '-pthread', '-ffp-contract=off', '-Wno-attributes', '-o', out,
                    os.path.join(tmp, 'episode_support.cpp')], check=True)
    lib = ctypes.CDLL(out)
    for name, (res, args) in _lib.SIGNATURES.items():
        if 'supp_loss' in name:
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib


def ptr(t):
    return None if t is None else t.data_ptr()


def run(lib, case, sim_target, thresh, present):
    X, c, x, sel = case['x'].contiguous(), case['confs'].contiguous(), case['logits'].contiguous(), case['sel']
    n, d = X.shape
    m = sel['proto'].numel()
    ws_floats = lib.effdet_episode_supp_loss_workspace_floats(n, d, m)
    ws = torch.zeros(ws_floats)
    idx = [sel['proto0'].contiguous(), sel['valid'].to(torch.uint8).contiguous(), sel['proto'].contiguous(), sel['nearest'].contiguous()]
    base = [None, ptr(X), ptr(c), ptr(x), n, d, m, case['dm'], case['da'], None] + [ptr(t) for t in idx] + [1 if sim_target == 'max' else 0]
    loss, target = torch.zeros(1), torch.zeros(n)
    assert lib.effdet_episode_supp_loss(*base, ptr(ws), ws_floats, ptr(loss), ptr(target)) == 0
    g = torch.tensor([case['g']], dtype=torch.float32)
    grads = [torch.zeros(n, d), torch.zeros(n), torch.zeros(n), torch.zeros(2)]
    assert lib.effdet_episode_supp_loss_backward(*base, thresh, ptr(g), ptr(ws), ws_floats, *[ptr(t) for t in grads]) == 0
    V = [(v.float().reshape(1) if v.dim() == 0 else v.float().contiguous()) if i in present else None for i, v in enumerate(case['V'])]
    d_g, hvp = torch.zeros(1), [torch.zeros(n, d), torch.zeros(n), torch.zeros(n), torch.zeros(2)]
    assert lib.effdet_episode_supp_loss_backward2(*base, thresh, ptr(g), *[ptr(v) for v in V], ptr(ws), ws_floats, ptr(d_g),
                                                  *[ptr(t) for t in hvp]) == 0
    split = lambda t: t[:3] + [t[3][0], t[3][1]]
    return loss[0], target, split(grads), d_g[0], split(hvp)


def main():
    worst = {'values': 0., 'first order': 0., 'second order': 0., 'E32': 0.}
    ok = True
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(tmp)
        for shape, sim_target, thresh, present in itertools.product(SHAPES, ('max', 'avg'), (1, 0), ((0, 1, 2, 3, 4), (2,), (0,))):
            num, rows, d, seed = shape
            for saturated, no_valid in ((False, False), (True, False), (False, True)):
                if (saturated or no_valid) and (shape != SHAPES[1] or present != (0, 1, 2, 3, 4)):
                    continue
                if no_valid and sim_target == 'max':
                    continue                                        # NaN by design; the GPU test checks that
                case = sref.draw(seed, num, rows, d, sim_target, saturated)
                if int(case['sel']['valid'].sum()) == 0:
                    case['sel'] = dict(case['sel'], valid=torch.ones_like(case['sel']['valid']))
                if no_valid:
                    case['sel'] = dict(case['sel'], valid=torch.zeros_like(case['sel']['valid']))
                w64 = sref.orders(case, 'lean', torch.float64, sim_target, bool(thresh), present=present)
                w32 = sref.orders(case, 'lean', torch.float32, sim_target, bool(thresh), present=present)
                loss, target, grads, d_g, hvp = run(lib, case, sim_target, thresh, present)
                line = []
                for kind, bound, pairs in (('values', 2e-5, [(loss, w64['loss'], None), (target, w64['target'], None)]),
                                           ('first order', 1e-4, [(a, b, None) for a, b in zip(grads, w64['grads'])]),
                                           ('second order', None, [(d_g, w64['d_g'], w32['d_g'])] +
                                            [(a, b, c) for a, b, c in zip(hvp, w64['hvp'], w32['hvp'])])):
                    rel = 0.
                    for got, want, want32 in pairs:
                        if want is None:
                            ok &= float(got.abs().max()) == 0.
                            continue
                        scale = float(want.abs().max())
                        err = float((got.double() - want).abs().max())
                        if bound is None:
                            e32 = float((want32.double() - want).abs().max())
                            worst['E32'] = max(worst['E32'], e32 / scale)
                            ok &= err <= 4 * e32 + 1e-7 * scale
                        else:
                            ok &= err <= bound * scale
                        rel = max(rel, err / scale)
                    worst[kind] = max(worst[kind], rel)
                    line.append('%s %.1e' % (kind, rel))
                print('%dx%d d%d %s thresh_grad=%d V=%s%s%s: %s' % (num, rows, d, sim_target, thresh, present, ' +-40' if saturated else '',
                                                                     ' no valid prototype' if no_valid else '', ', '.join(line)))
    print('largest error relative to the largest entry of the float64 form: ' + ', '.join('%s %.1e' % kv for kv in worst.items()))
    print('all within the bounds' if ok else 'A BOUND IS MISSED')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
