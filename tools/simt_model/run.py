#!/usr/bin/env python
"""episode.support_loss's kernels without a GPU: csrc/episode_support.hip compiled by g++ against the CPU model of common.h and
driven through the C ABI on CPU tensors, at all three orders, against the float64 lean form of tests/_support_loss_ref.py - the
comparison of tests/test_support_loss_gpu.py at its small shapes, with the same bounds (values 2e-5, gradients 1e-4, second order
4 E32 + 1e-7 of the largest entry).  Prints one line per configuration and the largest figures; exits 1 on a miss.

    python3 tools/simt_model/run.py            needs g++ with C++20 (std::barrier); a minute or so, a thread per lane

    python3 tools/simt_model/run.py --bits OUT --csrc DIR
compiles episode_loss.hip and episode_support.hip of DIR instead (default: this tree's csrc), runs every entry point of both through
the C ABI on the same shapes - both sim_targets, the three loss modes, thresh_grad 0 / 1, dots and cls_id by value and by pointer -
and writes one sha256 per output tensor to OUT (the workspace is not an output).  Two source trees whose files are identical
compute the same thing in the same order of operations; with the host's libm, so this compares structure, not the MI355X's bits."""
import argparse
import ctypes
import hashlib
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


CSRC = os.path.join(ROOT, 'ood_object_detection_amd', 'csrc')


def build(tmp, csrc=CSRC, unit='episode_support', entries='supp_loss'):
    shutil.copy(os.path.join(HERE, 'common.h'), tmp)
    shutil.copy(os.path.join(csrc, 'episode_rows.h'), tmp)
    shutil.copy(os.path.join(csrc, unit + '.hip'), os.path.join(tmp, unit + '.cpp'))
    out = os.path.join(tmp, 'lib%s_model.so' % unit)
    subprocess.run(['g++', '-std=c++20', '-O1', '-fPIC', '-shared', '-pthread', '-ffp-contract=off', '-Wno-attributes', '-o', out,
                    os.path.join(tmp, unit + '.cpp')], check=True)
    lib = ctypes.CDLL(out)
    for name, (res, args) in _lib.SIGNATURES.items():
        if entries in name:
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    return lib


def ptr(t):
    return None if t is None else t.data_ptr()


def run(lib, case, sim_target, thresh, present, dots=None):
    X, c, x, sel = case['x'].contiguous(), case['confs'].contiguous(), case['logits'].contiguous(), case['sel']
    n, d = X.shape
    m = sel['proto'].numel()
    ws_floats = lib.effdet_episode_supp_loss_workspace_floats(n, d, m)
    ws = torch.zeros(ws_floats)
    idx = [sel['proto0'].contiguous(), sel['valid'].to(torch.uint8).contiguous(), sel['proto'].contiguous(), sel['nearest'].contiguous()]
    base = [None, ptr(X), ptr(c), ptr(x), n, d, m, case['dm'], case['da'], ptr(dots)] + [ptr(t) for t in idx] + [1 if sim_target == 'max' else 0]
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


def run_proj(lib, case, labs, sim_target, mode, margin, by_pointer):
    """effdet_episode_proj_loss and its backward -> the seven output tensors"""
    import _episode_loss_ref as lref
    X, c, sel = case['x'].contiguous(), case['confs'].contiguous(), case['sel']
    n, d = X.shape
    m = sel['proto'].numel()
    ws_floats = lib.effdet_episode_proj_loss_workspace_floats(n, d, m)
    ws = torch.zeros(ws_floats)
    idx = [sel['proto0'].contiguous(), sel['valid'].to(torch.uint8).contiguous(), sel['proto'].contiguous(), sel['nearest'].contiguous()]
    dots = torch.tensor([case['dm'], case['da']], dtype=torch.float32) if by_pointer else None
    cls = torch.tensor([lref.CLS_ID], dtype=torch.int64) if by_pointer else None
    base = [None, ptr(X), ptr(c), ptr(labs), n, d, m, 0 if by_pointer else lref.CLS_ID, ptr(cls), 0. if by_pointer else case['dm'],
            0. if by_pointer else case['da'], ptr(dots)] + [ptr(t) for t in idx] + [1 if sim_target == 'max' else 0, mode, margin]
    losses, inner, stats, counts = torch.zeros(3), torch.zeros(n), torch.zeros(6), torch.zeros(3, dtype=torch.int32)
    assert lib.effdet_episode_proj_loss(*base, ptr(ws), ws_floats, ptr(losses), ptr(inner), ptr(stats), ptr(counts)) == 0
    gup = torch.tensor([0.7, case['g'], 0.01], dtype=torch.float32)
    grads = [torch.zeros(n, d), torch.zeros(n), torch.zeros(2)]
    assert lib.effdet_episode_proj_loss_backward(*base, ptr(gup), ptr(ws), ws_floats, *[ptr(t) for t in grads]) == 0
    return [losses, inner, stats, counts] + grads


def bits(out_path, csrc):
    """the --bits mode of the module docstring"""
    import _episode_loss_ref as lref
    sha = lambda t: hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest()
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        supp = build(tmp, csrc)
        proj = build(tmp, csrc, 'episode_loss', 'proj_loss')
        for (num, rows, d, seed), sim_target, by_pointer in itertools.product(SHAPES, ('max', 'avg'), (False, True)):
            case = sref.draw(seed, num, rows, d, sim_target)
            what = '%dx%d d%d %s %s' % (num, rows, d, sim_target, 'by pointer' if by_pointer else 'by value')
            labs = lref.draw_labels(seed, num * rows, True)
            for mode, name in enumerate(('separate', 'same', 'no_conf')):
                for i, t in enumerate(run_proj(proj, case, labs, sim_target, mode, 0.1, by_pointer)):
                    lines.append('proj_loss %s %s %d %s' % (what, name, i, sha(t)))
            dots = torch.tensor([case['dm'], case['da']], dtype=torch.float32) if by_pointer else None
            for thresh in (1, 0):
                loss, target, grads, d_g, hvp = run(supp, case, sim_target, thresh, (0, 1, 2, 3, 4), dots)
                for i, t in enumerate([loss, target, d_g] + grads + hvp):
                    lines.append('supp_loss %s thresh_grad=%d %d %s' % (what, thresh, i, sha(t)))
            print(what, flush=True)
    with open(out_path, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('%d digests -> %s' % (len(lines), out_path))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--bits', metavar='OUT', help='write a sha256 per output tensor of every entry point instead of comparing')
    ap.add_argument('--csrc', metavar='DIR', default=CSRC, help='the directory whose episode sources --bits compiles')
    a = ap.parse_args()
    if a.bits:
        return bits(a.bits, a.csrc)
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
