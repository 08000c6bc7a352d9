"""The yardsticks of tests/test_support_loss_gpu.py checked against each other on the CPU, and the parts of
episode.support_loss's C ABI that answer without a GPU."""
import pytest
import torch

import _support_loss_ref as sref

CASES = [(5, 37, 24, 6), (7, 20, 16, 3)]              # num, rows, d, seed


def _agree(a, b, what):
    assert (a is None) == (b is None), what
    if a is None:
        return
    scale = float(b.abs().max())
    err = float((a - b).abs().max())
    print('%s: max err %.3e, largest entry %.3e' % (what, err, scale))
    assert err <= 1e-12 * scale, (what, err, scale)


@pytest.mark.parametrize('thresh_grad', [True, False])
@pytest.mark.parametrize('sim_target', ['max', 'avg'])
@pytest.mark.parametrize('num,rows,d,seed', CASES)
def test_lean_form_equals_the_literal_form_at_every_order(num, rows, d, seed, sim_target, thresh_grad):
    case = sref.draw(seed, num, rows, d, sim_target)
    assert int(case['sel']['valid'].sum()) >= 2
    lean = sref.orders(case, 'lean', torch.float64, sim_target, thresh_grad)
    lit = sref.orders(case, 'literal', torch.float64, sim_target, thresh_grad)
    _agree(lean['loss'], lit['loss'], 'loss')
    _agree(lean['target'], lit['target'], 'target')
    _agree(lean['d_g'], lit['d_g'], 'd g')
    for i, name in enumerate(sref.NAMES):
        _agree(lean['grads'][i], lit['grads'][i], 'gradient ' + name)
        _agree(lean['hvp'][i], lit['hvp'][i], 'hvp ' + name)
    if not thresh_grad:
        assert all(lean['grads'][i] is None for i in (1, 3, 4))


def test_shared_head_adds_the_two_gradients():
    case = sref.draw(6, 5, 37, 24, 'max')
    both = sref.orders(case, 'lean', torch.float64, shared_head=True, second=False)
    case2 = dict(case, logits=case['confs'])
    apart = sref.orders(case2, 'lean', torch.float64, second=False)
    _agree(both['grads'][1], apart['grads'][1] + apart['grads'][2], 'confs is logits')


def test_workspace_query_answers_and_refuses():
    from ood_object_detection_amd import _lib
    lib = _lib.load()
    for name in ('effdet_episode_supp_loss', 'effdet_episode_supp_loss_backward', 'effdet_episode_supp_loss_backward2'):
        assert hasattr(lib, name), name
    query = lib.effdet_episode_supp_loss_workspace_floats
    assert query(6300, 256, 25) > 0
    assert query(6400, 512, 33) == -1                  # m d > 16384
    assert query(10, 8, 11) == -1                      # n < m
    assert query(8, 520, 2) == -1                      # d > 512
    assert query(8, 8, 65) == -1                       # m > 64
    assert lib.effdet_abi_version() == 1
