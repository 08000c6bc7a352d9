"""ood_train without a GPU: the float64 restatement of tests/_energy_reg_ref.py against torch.autograd on the literal float64
composition, `anchor_roles` on a hand-written example, and the argument checks of `EnergyRegularizer`."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _energy_reg_ref as R


def _literal(z, role, form, kind, T, m_in, m_out, w_in, w_out, min_max, phi):
    """the loss as a user would compose it from torch ops, float64 on the CPU -> loss, d loss / d z, d loss / d (w, b)"""
    z = torch.from_numpy(z.astype(np.float64)).requires_grad_()
    w = torch.tensor(float(np.float32(phi[0])), dtype=torch.float64, requires_grad=True)
    b = torch.tensor(float(np.float32(phi[1])), dtype=torch.float64, requires_grad=True)
    role = torch.from_numpy(role.astype(np.int64))
    E = -T * torch.logsumexp(z / T, -1) if kind == 'logsumexp' else -F.softplus(z).sum(-1)
    is_in, is_out = role == 1, role == 0
    if min_max is not None:
        is_out = is_out & (z.detach().max(-1).values >= float(np.float32(min_max)))
    if form == 'hinge':
        l_in, l_out = (E - m_in).relu() ** 2, (m_out - E).relu() ** 2
    else:
        s = w * (-E) + b
        l_in, l_out = F.softplus(-s), F.softplus(s)
    zero = torch.zeros((), dtype=torch.float64)
    loss = w_in * (l_in[is_in].mean() if bool(is_in.any()) else zero) + w_out * (l_out[is_out].mean() if bool(is_out.any()) else zero)
    if not loss.requires_grad:                                   # both sides empty
        return 0.0, np.zeros(z.shape), np.zeros(2)
    gz, gw, gb = torch.autograd.grad(loss, [z, w, b], allow_unused=True)
    g = lambda t: 0.0 if t is None else float(t)
    return float(loss), gz.numpy(), np.array([g(gw), g(gb)])


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize('form', R.FORMS)
@pytest.mark.parametrize('kind,T', [('logsumexp', 1.0), ('logsumexp', 2.5), ('joint', 1.0)])
@pytest.mark.parametrize('case', ['plain', 'no outliers', 'no in-distribution', 'filter'])
def test_restatement_against_autograd(form, kind, T, case):
    C, n = 7, 40
    z, role = R.inputs(C, n)
    if case == 'no outliers':
        role[role == 0] = -1
    if case == 'no in-distribution':
        role[role == 1] = 3
    min_max = float(np.median(z[role == 0].max(1))) if case == 'filter' else None
    E = R.energy(z, kind, T)[0]
    kw = dict(form=form, kind=kind, T=T, m_in=float(np.float32(np.median(E))), m_out=float(np.float32(np.median(E) + 0.5)), w_in=0.75,
              w_out=1.5, min_max=min_max, phi=(0.5, -1.25))
    ref = R.forward(z, role, **kw)
    loss, gz, gphi = _literal(z, role, **kw)
    assert ref['n_in'] == (0 if case == 'no in-distribution' else int((role == 1).sum()))
    if case == 'filter':
        assert 0 < ref['n_out'] < int((role == 0).sum())
        assert ref['n_out'] == int((z[role == 0].max(1) >= np.float32(min_max)).sum())
    assert abs(ref['loss'] - loss) <= 1e-12 * abs(loss)
    assert _rel(ref['grad_logits'], gz) <= 1e-12
    assert not ref['grad_logits'][ref['side'] == 0].any()
    if form == 'logistic':
        assert _rel(ref['grad_phi'], gphi) <= 1e-12
    else:
        assert not ref['grad_phi'].any() and (ref['n_in'] == 0 or 0 < ref['active_in'] < ref['n_in'])
    # the float32 yardstick follows the reference closely, and a row that does not count changes nothing
    f32 = R.forward(z, role, dtype=np.float32, **kw)
    assert abs(float(f32['loss']) - ref['loss']) <= 1e-5 * max(abs(ref['loss']), 1e-3)
    z2 = z.copy()
    z2[ref['side'] == 0] = np.nan
    again = R.forward(z2, role, **kw)
    assert again['loss'] == ref['loss'] and np.array_equal(again['grad_logits'], ref['grad_logits'])


def test_anchor_roles_on_a_hand_written_example():
    from ood_object_detection_amd.ood_train import anchor_roles
    cls_t = torch.tensor([[3, -1, -2, 0, -1],          # an in-distribution image
                          [-1, 5, -2, -1, -1],         # an outlier image that contains a positive label
                          [-2, -2, -1, -1, 7]])        # an in-distribution image
    outlier = torch.tensor([False, True, False])
    none = anchor_roles(cls_t, outlier)
    assert none.dtype == torch.int8 and none.tolist() == [[1, -1, -1, 1, -1], [0, 0, -1, 0, 0], [-1, -1, -1, -1, 1]]
    bg = anchor_roles(cls_t, outlier, background='outlier')
    assert bg.tolist() == [[1, 0, -1, 1, 0], [0, 0, -1, 0, 0], [-1, -1, 0, 0, 1]]
    # the per-level list of the labeler ([B, H, W, A]) packs to the same anchors
    levels = [cls_t[:, :4].reshape(3, 2, 1, 2), cls_t[:, 4:].reshape(3, 1, 1, 1)]
    assert torch.equal(anchor_roles(levels, outlier, 'outlier'), bg)
    with pytest.raises(ValueError):
        anchor_roles(cls_t, outlier, background='all')
    with pytest.raises(ValueError):
        anchor_roles(cls_t, outlier[:2])
    with pytest.raises(ValueError):
        anchor_roles(cls_t, outlier.to(torch.int64))


def test_argument_checks():
    from ood_object_detection_amd.ood_train import EnergyRegularizer
    with pytest.raises(ValueError, match='margin'):
        EnergyRegularizer(7, 'hinge')
    with pytest.raises(ValueError, match='margin'):
        EnergyRegularizer(7, 'hinge', margin_in=-5.0)
    with pytest.raises(ValueError, match='temperature'):
        EnergyRegularizer(7, 'logistic', energy='joint', temperature=2.0)
    with pytest.raises(ValueError, match='temperature'):
        EnergyRegularizer(7, 'logistic', temperature=0.0)
    for C in (0, 1025):
        with pytest.raises(ValueError, match='num_classes'):
            EnergyRegularizer(C, 'logistic')
    with pytest.raises(ValueError):
        EnergyRegularizer(7, 'focal')
    with pytest.raises(ValueError):
        EnergyRegularizer(7, 'logistic', energy='free')
    with pytest.raises(ValueError):
        EnergyRegularizer(7, 'logistic', min_max_logit=float('nan'))
    reg = EnergyRegularizer(7, 'logistic')
    assert isinstance(reg, torch.nn.Module) and [tuple(p.shape) for p in reg.parameters()] == [(2,)] and reg.phi.tolist() == [1.0, 0.0]
    hinge = EnergyRegularizer(7, 'hinge', margin_in=-5.0, margin_out=-1.0)
    assert list(hinge.parameters()) == []
    roles = torch.zeros(2, 5, dtype=torch.int8)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        reg(torch.zeros(2, 5, 7), roles)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        reg([torch.zeros(2, 14, 1, 1)], roles)


def test_roles_shape_and_dtype_are_checked_before_any_launch(monkeypatch):
    """(the checks run before the library is touched: a stand-in device type lets them run without a GPU)"""
    from ood_object_detection_amd import ood_train
    reg = ood_train.EnergyRegularizer(7, 'logistic')
    monkeypatch.setattr(ood_train.EnergyRegularizer, '_logits', lambda self, t: t)
    z = torch.zeros(2, 5, 7)
    with pytest.raises(ValueError, match='int8'):
        reg(z, torch.zeros(2, 5, dtype=torch.int64))
    with pytest.raises(ValueError, match=r'\[2, 5\]'):
        reg(z, torch.zeros(2, 4, dtype=torch.int8))
    with pytest.raises(ValueError, match=r'\[2, 5\]'):
        reg(z, torch.zeros(10, dtype=torch.int8))
