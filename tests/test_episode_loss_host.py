"""Host-side checks of episode.projection_losses (no GPU): the entry points are declared, bound and exported; the workspace query's
limits; CPU tensors and unknown modes are refused; and the lean float64 form of tests/_episode_loss_ref.py - the yardstick of the GPU
tests - equals the literal n x n form of infer.py:448-494, values and gradients."""
import ctypes
import itertools
import os
import re

import pytest
import torch

import _episode_loss_ref as lref
import _episode_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {'effdet_episode_proj_loss_workspace_floats': 3, 'effdet_episode_proj_loss': 25, 'effdet_episode_proj_loss_backward': 25}


def test_proj_loss_entry_points_declared_bound_and_exported():
    from ood_object_detection_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'effdet_hip.h')).read()
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    import torch  # noqa: F401  (share torch's HIP runtime, see _lib.load)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in ENTRY_POINTS.items():
        found = re.search(r'\b(int|long long)\s+%s\s*\(([^;]*)\)\s*;' % name, header)
        assert found, name
        assert len(found.group(2).split(',')) == nargs, name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
        assert hasattr(lib, name), name
    q = lib.effdet_episode_proj_loss_workspace_floats
    q.restype = ctypes.c_longlong
    n, d, m = 42300, 256, 25
    assert 3 * n < q(n, d, m) < 8 * n + 40 * m * d                  # O(n + parts * m * d), pure host arithmetic
    assert q(320, 256, 64) > 0 and q(37 * 5, 100, 5) > 0 and q(64, 256, 64) > 0
    assert q(6500, 256, 65) == -1                                     # m > 64
    assert q(6400, 512, 33) == -1                                     # m * d > 16384
    assert q(6400, 513, 2) == -1                                      # d > 512
    assert q(24, 256, 25) == -1 and q(0, 256, 25) == -1 and q(100, 0, 5) == -1 and q(100, 8, 0) == -1


def test_cpu_tensors_and_unknown_modes_raise():
    from ood_object_detection_amd import episode
    n, m = 10, 2
    sel = dict(proto0=torch.zeros(m, dtype=torch.int64), valid=torch.ones(m, dtype=torch.bool), proto=torch.zeros(m, dtype=torch.int64),
               nearest=torch.zeros(n, dtype=torch.int64))
    args = (torch.zeros(n, 8), torch.zeros(n), torch.zeros(n, dtype=torch.int64), 1, sel, 1.0, 0.0)
    with pytest.raises(RuntimeError):
        episode.projection_losses(*args)
    with pytest.raises(ValueError):
        episode.projection_losses(*args, sim_target='median')
    with pytest.raises(ValueError):
        episode.projection_losses(*args, loss_mode='both')
    with pytest.raises(RuntimeError):
        episode.projection_losses(torch.zeros(n, 8, dtype=torch.float64), *args[1:])


CONFIGS = [('max', 'separate'), ('max', 'same'), ('max', 'no_conf'), ('avg', 'separate')]


@pytest.mark.parametrize('num,rows,d,seed', [(7, 100, 64, 3), (5, 37, 100, 6)])
def test_lean_form_equals_literal_form(num, rows, d, seed):
    x, confs = ref.clustered_rows(seed, num, rows, d)
    confs = torch.randn(confs.shape, generator=torch.Generator().manual_seed(seed))
    n = num * rows
    for (sim_target, loss_mode), margin, first in itertools.product(CONFIGS, (0., 0.1), (True, False)):
        labs = lref.draw_labels(seed, n, first)
        sel, _ = lref.decisions(x.double(), confs.double(), 1.5, 0.25, num, sim_target)
        assert int(sel['valid'].sum()) >= 3
        leaves = [[t.clone().requires_grad_() for t in (x.double(), confs.double(), torch.tensor(1.5, dtype=torch.float64),
                                                       torch.tensor(0.25, dtype=torch.float64))] for _ in range(2)]
        outs = [f(lv[0], lv[1], labs, lref.CLS_ID, sel, lv[2], lv[3], sim_target, loss_mode, margin)
                for f, lv in zip((lref.losses_literal, lref.losses_lean), leaves)]
        lit, lean = outs
        what = (sim_target, loss_mode, margin, first)
        if not first and sim_target == 'max':
            assert lit['positives'] == lean['positives'] == 0, what         # labs[0] is not the task class: no positive embds target
        elif first:
            assert lit['positives'] == lean['positives'] > 0, what
        assert lit['counts'] == lean['counts'] and min(lit['counts']) > 0
        for k in ('clust_loss', 'embds_loss', 'obj_loss', 'inner_target'):
            assert float((lit[k].detach() - lean[k].detach()).abs().max()) <= 1e-12, (what, k)
        for k in lref.STAT_NAMES:
            assert float((lit['stats'][k] - lean['stats'][k]).abs()) <= 1e-12, (what, k)
        grads = [torch.autograd.grad(0.7 * (o['clust_loss'] + o['embds_loss']) + 0.01 * o['obj_loss'], lv) for o, lv in zip(outs, leaves)]
        for g_lit, g_lean in zip(*grads):
            scale = float(g_lit.abs().max())
            assert scale > 0 and float((g_lit - g_lean).abs().max()) <= 1e-12 * scale, what
