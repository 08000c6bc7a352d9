"""ood_train.EnergyRegularizer (csrc/energy_reg.hip) against the numpy restatement of tests/_energy_reg_ref.py, and its hook in
pretrain.PretrainStep.

Inputs (`_energy_reg_ref.inputs`): logits 2 N(0, 1) - 3 with +5 on one random class of every in-distribution row, rounded to float32;
roles drawn from (1, 0, -1).  B = 3; N in {1, 5, 16, 17, 67} (around the 16-row workgroup); C in {1, 2, 7, 63, 64, 65, 90, 128, 129,
300, 1024} (the lane slice at 64 and every instantiation boundary).  The hinge's margins are the medians of the float64 reference
energy of each side, rounded to float32, so about half the rows of a side have an active hinge: both shares lie in [0.25, 0.75]
whenever a side has at least 8 rows (asserted).

Bounds.  Per-row energy, grad_logits and grad_phi: within 4 E32 + 1e-7 max |value| of the float64 restatement, per key and case; E32
is the float32 restatement's own error on the same inputs.  mean_l / mean_energy per side: the same bound formed from that side's
per-row l / E (a float64 mean of terms each within a bound cannot be farther); loss: |weight_in| bound(l in) + |weight_out| bound(l
out).  No row is left out of a comparison.  n_in and n_out are exact.  The active counts are exact for every row the reference can
decide: the median of an odd number of energies IS one row's energy, so that one row has d = 0 up to the rounding of the margin and
sits on the hinge's kink (|d| below the case's energy bound); it may count as active or not, and there is at most one such row per
side (asserted, `_energy_reg_ref.active_ranges`).  Every case prints E32, the device error and the bound before it asserts.
Measured on an MI355X: see the accuracy table of DESIGN.md §8."""
import numpy as np
import pytest
import torch

import _energy_reg_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
B = 3
ROWS_N = (1, 5, 16, 17, 67)
CLASSES = (1, 2, 7, 63, 64, 65, 90, 128, 129, 300, 1024)
VARIANTS = [(f, k, T) for f in R.FORMS for k, T in (('logsumexp', 1.0), ('logsumexp', 2.5), ('joint', 1.0))]
W_IN, W_OUT, PHI = 0.75, 1.5, (0.5, -1.25)


def _reg(C, form, kind='logsumexp', T=1.0, m_in=None, m_out=None, min_max=None, w_in=W_IN, w_out=W_OUT, phi=PHI):
    from ood_object_detection_amd.ood_train import EnergyRegularizer
    reg = EnergyRegularizer(C, form, energy=kind, temperature=T, margin_in=m_in, margin_out=m_out, weight_in=w_in, weight_out=w_out,
                            min_max_logit=min_max).to(DEV)
    if form == 'logistic':
        with torch.no_grad():
            reg.phi.copy_(torch.tensor(phi))
    return reg


def _run(reg, z, roles, upstream=None):
    """forward + backward -> dict of the outputs (device tensors); z: [B, N, C] tensor or a per-level list built from a leaf"""
    leaf = z if torch.is_tensor(z) else None
    if leaf is not None:
        leaf = leaf.detach().clone().requires_grad_()
        z = leaf
    if reg.phi is not None:
        reg.phi.grad = None
    loss, stats = reg(z, roles, return_energy=True)
    if leaf is not None:
        (loss if upstream is None else loss * upstream).backward()
    out = dict(stats, loss=loss.detach())
    out['grad_logits'] = None if leaf is None else leaf.grad
    out['grad_phi'] = torch.zeros(2, device=DEV) if reg.phi is None or reg.phi.grad is None else reg.phi.grad.clone()
    return out


def _eq(a, b, skip=()):
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a if k not in skip)


def _margins(z, role, kind, T):
    E = R.energy(z, kind, T)[0]
    med = lambda v: float(np.float32(np.median(v))) if len(v) else 0.0
    return med(E[role == 1]), med(E[role == 0])


def _check(got, ref, f32, name):
    bnd = R.bounds(ref, f32, W_IN, W_OUT)
    n, C = ref['grad_logits'].shape
    worst = {}
    for k in ('energy', 'grad_logits', 'grad_phi', 'loss', 'mean_l_in', 'mean_l_out', 'mean_energy_in', 'mean_energy_out'):
        dev = got[k].double().cpu().numpy().reshape(np.shape(ref[k]))
        err = float(np.abs(dev - ref[k]).max())
        e32, b = bnd[k]
        print('%s %s: max |value| %.3g, device error %.2e, E32 %.2e, bound %.2e' % (name, k, float(np.abs(ref[k]).max()), err, e32, b))
        assert err <= b, (name, k, err, b)
        worst[k] = (err, e32, b)
    assert int(got['n_in']) == ref['n_in'] and int(got['n_out']) == ref['n_out'], name
    act = R.active_ranges(ref, bnd['energy'][1])
    for side in ('in', 'out'):
        lo, hi = act[side]
        a = int(got['active_' + side])
        assert hi <= lo + 1 and lo <= a <= hi, (name, side, a, act[side])
        cnt = ref['n_' + side]
        if ref['form'] == 'hinge' and cnt >= 8:
            assert 0.25 <= a / cnt <= 0.75, (name, side, a, cnt)
    dead = torch.from_numpy(ref['side'] == 0).to(DEV)
    assert not bool(got['energy'].reshape(n)[dead].any()) and not bool(got['grad_logits'].reshape(n, C)[dead].any()), name
    return worst


# ---- accuracy -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form,kind,T', VARIANTS)
@pytest.mark.parametrize('C', CLASSES)
def test_accuracy(C, form, kind, T):
    table, missed = {}, []
    for N in ROWS_N:
        z, role = R.inputs(C, B * N)
        m_in, m_out = _margins(z, role, kind, T)
        filters = (None, float(np.median(z[role == 0].max(1)))) if N == 67 else (None,)
        for min_max in filters:
            kw = dict(form=form, kind=kind, T=T, m_in=m_in, m_out=m_out, w_in=W_IN, w_out=W_OUT, min_max=min_max, phi=PHI)
            if min_max is not None:                              # the margin of the rows the filter keeps
                kept = R.sides(z, role, min_max) == 2
                kw['m_out'] = float(np.float32(np.median(R.energy(z[kept], kind, T)[0])))
                assert 0 < kept.sum() < (role == 0).sum()
            ref, f32 = R.forward(z, role, **kw), R.forward(z, role, dtype=np.float32, **kw)
            reg = _reg(C, form, kind, T, kw['m_in'], kw['m_out'], min_max)
            got = _run(reg, torch.from_numpy(z).to(DEV).reshape(B, N, C), torch.from_numpy(role).to(DEV).reshape(B, N))
            torch.cuda.synchronize()
            assert got['energy'].shape == (B, N) and got['energy'].dtype == torch.float32 and got['grad_logits'].shape == (B, N, C)
            assert got['loss'].dtype == torch.float32 and got['loss'].dim() == 0 and got['n_in'].dtype == torch.int64
            try:                                                 # (every N is measured before the test fails)
                w = _check(got, ref, f32, 'C %d %s %s T %.1f N %d%s' % (C, form, kind, T, N, '' if min_max is None else ' filtered'))
            except AssertionError as e:
                missed.append(e.args[0])
                continue
            for k, v in w.items():
                if k not in table or v[0] / max(v[2], 1e-300) > table[k][0] / max(table[k][2], 1e-300):
                    table[k] = v
    print('TABLE C %d %s %s T %.1f: %s' % (C, form, kind, T, '; '.join('%s err %.2e E32 %.2e bound %.2e' % ((k,) + v) for k, v in table.items())))
    assert not missed, missed


# ---- edges ------------------------------------------------------------------------------------------------------------------------
def _case(C, N, form, kind, T=1.0, min_max=None):
    z, role = R.inputs(C, B * N, seed=3)
    m_in, m_out = _margins(z, role, kind, T)
    return z, role, _reg(C, form, kind, T, m_in, m_out, min_max)


def _dev(z, role, N, dtype=torch.float32):
    C = z.shape[1]
    return torch.from_numpy(z).to(DEV).reshape(B, N, C).to(dtype), torch.from_numpy(role).to(DEV).reshape(B, N)


@pytest.mark.parametrize('form,kind', [('hinge', 'logsumexp'), ('logistic', 'joint')])
def test_no_row_counts_and_an_empty_side(form, kind):
    C, N = 90, 17
    z, role, reg = _case(C, N, form, kind)
    zt, rt = _dev(z, role, N)
    none = _run(reg, zt, torch.full_like(rt, -1))
    assert float(none['loss']) == 0.0 and not bool(none['grad_logits'].any()) and not bool(none['energy'].any()) and not bool(none['grad_phi'].any())
    for k in ('n_in', 'n_out', 'active_in', 'active_out', 'mean_l_in', 'mean_l_out', 'mean_energy_in', 'mean_energy_out'):
        assert float(none[k]) == 0.0, k
    seven = _run(reg, zt, torch.full_like(rt, 7))              # "anything else": not a role
    assert _eq(seven, none)
    for drop, empty, other in ((0, 'out', 'in'), (1, 'in', 'out')):
        r1 = role.copy()
        r1[r1 == drop] = -1
        kw = dict(form=form, kind=kind, m_in=reg.margin_in, m_out=reg.margin_out, w_in=W_IN, w_out=W_OUT, phi=PHI)
        ref, f32 = R.forward(z, r1, **kw), R.forward(z, r1, dtype=np.float32, **kw)
        got = _run(reg, zt, torch.from_numpy(r1).to(DEV).reshape(B, N))
        assert int(got['n_' + empty]) == 0 and float(got['mean_l_' + empty]) == 0.0 and int(got['n_' + other]) > 0
        _check(got, ref, f32, '%s %s empty %s' % (form, kind, empty))


@pytest.mark.parametrize('form,kind,T', VARIANTS)
def test_extreme_logits_stay_finite_and_a_nan_stays_in_its_row(form, kind, T):
    C, N = 90, 17
    z, role, _ = _case(C, N, form, kind, T)
    thr = float(np.median(z[role == 0].max(1)))
    reg = _reg(C, form, kind, T, -1.0, -3.0, thr)
    side = R.sides(z, role, thr)
    cin, cout = np.nonzero(side == 1)[0], np.nonzero(side == 2)[0]
    dead, rejected = np.nonzero(role == -1)[0], np.nonzero((role == 0) & (side == 0))[0]
    assert min(len(cin), len(cout)) >= 2 and len(dead) >= 1 and len(rejected) >= 1
    z = z.copy()
    z[cin[0]], z[cin[1]], z[cout[0]], z[cout[1]] = 80.0, -80.0, 80.0, 80.0
    z[cout[1], 1:] = -80.0                                      # (at C > 1: +80 and -80 in one row)
    zt, rt = _dev(z, role, N)
    a = _run(reg, zt, rt)
    torch.cuda.synchronize()
    for k, v in a.items():
        assert bool(torch.isfinite(v.double()).all()), k
    assert int(a['n_in']) == len(cin) and int(a['n_out']) == len(cout)
    # a NaN in a row that does not count, and in an outlier row the filter rejects: as if the row held zeros, bit for bit
    # (the rejected row's maximum is below the threshold, which is positive: a row of zeros is rejected as well)
    assert thr > 0
    zn, z0 = z.copy(), z.copy()
    zn[dead[0], C // 2], zn[rejected[0], 0] = np.nan, np.nan
    z0[dead[0]], z0[rejected[0]] = 0.0, 0.0
    assert _eq(_run(reg, _dev(zn, role, N)[0], rt), _run(reg, _dev(z0, role, N)[0], rt))
    assert _eq(_run(reg, _dev(zn, role, N)[0], rt), a)
    # a NaN in a counted row: a NaN loss; the other rows keep their bits
    zc = z.copy()
    zc[cin[2 % len(cin)], C - 1] = np.nan
    b = _run(reg, _dev(zc, role, N)[0], rt)
    assert bool(torch.isnan(b['loss']))
    keep = torch.arange(B * N, device=DEV) != int(cin[2 % len(cin)])
    assert torch.equal(a['energy'].reshape(-1)[keep], b['energy'].reshape(-1)[keep])
    assert torch.equal(a['grad_logits'].reshape(B * N, C)[keep], b['grad_logits'].reshape(B * N, C)[keep])
    assert int(b['n_in']) == len(cin) and int(b['n_out']) == len(cout)
    # without a filter a NaN outlier row counts (and spoils the loss); with one it has no maximum and is rejected
    zo = z.copy()
    zo[cout[0], 0] = np.nan
    c = _run(reg, _dev(zo, role, N)[0], rt)
    assert int(c['n_out']) == len(cout) - 1 and bool(torch.isfinite(c['loss']))


def test_a_row_whose_maximum_equals_min_max_logit_counts():
    C, N = 90, 17
    z, role, _ = _case(C, N, 'hinge', 'logsumexp')
    out = np.nonzero(role == 0)[0]
    mz = z[out].max(1)
    thr = float(np.sort(mz)[len(mz) // 2])                      # one row's exact float32 maximum
    reg = _reg(C, 'hinge', 'logsumexp', 1.0, -1.0, -3.0, thr)
    got = _run(reg, *_dev(z, role, N))
    assert int(got['n_out']) == int((mz >= np.float32(thr)).sum()) and int((mz == np.float32(thr)).sum()) == 1
    above = _reg(C, 'hinge', 'logsumexp', 1.0, -1.0, -3.0, float(np.nextafter(np.float32(thr), np.float32(np.inf))))
    assert int(_run(above, *_dev(z, role, N))['n_out']) == int(got['n_out']) - 1
    row = int(out[np.nonzero(mz == np.float32(thr))[0][0]])
    assert float(got['energy'].reshape(-1)[row]) != 0.0 and float(_run(above, *_dev(z, role, N))['energy'].reshape(-1)[row]) == 0.0


# ---- bitwise ------------------------------------------------------------------------------------------------------------------------
def _levels_of(packed, C, A=3, hw=((4, 3), (2, 2), (1, 1))):
    """a packed [B, N, C] tensor (N = A * cells) -> the per-level [B, A * C, H, W] list of the class head"""
    out, at = [], 0
    for h, w in hw:
        n = h * w * A
        out.append(packed[:, at:at + n].reshape(packed.shape[0], h, w, A * C).permute(0, 3, 1, 2))
        at += n
    assert at == packed.shape[1]
    return out


@pytest.mark.parametrize('form,kind,T', VARIANTS)
@pytest.mark.parametrize('C', [7, 90, 300])
def test_bitwise_pairs(C, form, kind, T):
    N = 51                                                       # 3 anchors * (12 + 4 + 1) cells
    z, role, reg = _case(C, N, form, kind, T)
    zt, rt = _dev(z, role, N)
    base = _run(reg, zt, rt)
    assert _eq(base, _run(reg, zt, rt)), 'two runs'
    # the per-level list against the packed tensor (the gradient arrives through the packing)
    leaf = zt.clone().requires_grad_()
    loss, stats = reg(_levels_of(leaf, C), rt, return_energy=True)
    loss.backward()
    assert torch.equal(loss.detach(), base['loss']) and all(torch.equal(stats[k], base[k]) for k in stats)
    assert torch.equal(leaf.grad, base['grad_logits'])
    leaf = zt.clone().requires_grad_()                          # levels with storage of their own: the packing concatenates
    loss, stats = reg([t.clone() for t in _levels_of(leaf, C)], rt, return_energy=True)
    loss.backward()
    assert torch.equal(loss.detach(), base['loss']) and all(torch.equal(stats[k], base[k]) for k in stats)
    assert torch.equal(leaf.grad, base['grad_logits'])
    # bfloat16 logits against their float32 widening; grad_logits after rounding to bfloat16
    zb = zt.to(torch.bfloat16)
    gb, gw = _run(reg, zb, rt), _run(reg, zb.float(), rt)
    assert gb['grad_logits'].dtype == torch.bfloat16 and _eq(gb, gw, skip=('grad_logits',))
    assert torch.equal(gb['grad_logits'], gw['grad_logits'].to(torch.bfloat16))


@pytest.mark.parametrize('form,kind', [('hinge', 'logsumexp'), ('logistic', 'joint')])
def test_graph_replay_of_forward_and_backward(form, kind):
    C, N = 90, 67
    z, role, reg = _case(C, N, form, kind)
    zt, rt = _dev(z, role, N)
    eager = _run(reg, zt, rt)
    s_z = torch.zeros_like(zt).requires_grad_()
    s_r = torch.full_like(rt, -1)
    if reg.phi is not None:
        reg.phi.grad = torch.zeros_like(reg.phi)
    s_z.grad = torch.zeros_like(s_z)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            s_z.grad.zero_()
            if reg.phi is not None:
                reg.phi.grad.zero_()
            loss, stats = reg(s_z, s_r, return_energy=True)
            loss.backward()
    torch.cuda.current_stream(DEV).wait_stream(side)
    with torch.no_grad():
        s_z.copy_(zt)
    s_r.copy_(rt)
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss.detach(), eager['loss']) and all(torch.equal(stats[k], eager[k]) for k in stats)
        assert torch.equal(s_z.grad, eager['grad_logits'])
        if reg.phi is not None:
            assert torch.equal(reg.phi.grad, eager['grad_phi'])


# ---- autograd -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', R.FORMS)
def test_autograd(form):
    C, N = 90, 17
    z, role, reg = _case(C, N, form, 'logsumexp')
    zt, rt = _dev(z, role, N)
    one = _run(reg, zt, rt)
    three = _run(reg, zt, rt, upstream=3.0)
    assert torch.equal(three['grad_logits'], one['grad_logits'] * 3.0) and bool(one['grad_logits'].any())
    if form == 'logistic':
        assert bool(one['grad_phi'].all()) and torch.equal(three['grad_phi'], one['grad_phi'] * 3.0)
    else:
        assert reg.phi is None and list(reg.parameters()) == []
    # without a gradient to compute nothing else changes
    with torch.no_grad():
        loss, stats = reg(zt, rt)
    assert torch.equal(loss, one['loss']) and 'energy' not in stats and not loss.requires_grad
    # a second backward through the same graph raises, and so does differentiating twice (no second-order backward is built)
    leaf = zt.clone().requires_grad_()
    loss, _ = reg(leaf, rt)
    loss.backward()
    with pytest.raises(RuntimeError):
        loss.backward()
    leaf = zt.clone().requires_grad_()
    loss, _ = reg(leaf, rt)
    g, = torch.autograd.grad(loss, leaf, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()
    with pytest.raises(ValueError):
        reg(zt, rt.to(torch.int64))
    with pytest.raises(ValueError):
        reg(zt, rt[:, :5])
    with pytest.raises(ValueError):
        reg(zt[:, :, :7], rt)
    with pytest.raises(RuntimeError):
        reg(zt.double(), rt)


# ---- PretrainStep -------------------------------------------------------------------------------------------------------------------
SIZE, PB, PC = 128, 2, 20


def _pretrain_inputs(steps):
    g = torch.Generator().manual_seed(3)
    xs = [torch.randint(0, 256, (PB, 3, SIZE, SIZE), generator=g, dtype=torch.uint8).to(DEV) for _ in range(steps)]
    boxes = [torch.tensor([[10., 12., 70., 90.], [40., 30., 120., 100.]]), torch.tensor([[5., 5., 60., 50.]])]
    cls = [torch.tensor([3, 7]), torch.tensor([1])]
    target = {'bbox': [b.to(DEV) for b in boxes], 'cls': [c.to(DEV) for c in cls], 'outlier': torch.tensor([False, True], device=DEV)}
    return xs, target


def _model():
    from _models import seeded_model
    model, cfg, _, _ = seeded_model('tf_efficientdet_d0', SIZE, PC, seed=23)
    return model.to(DEV).float()


def _state(model):
    return {n: p.detach().clone() for n, p in model.named_parameters()}, {n: b.detach().clone() for n, b in model.named_buffers()}


def _hinge(**kw):
    # margins far on either side of the energies of the seeded head (a few units around zero) keep both hinges active in every row
    # whatever the weights do in four steps
    return _reg(PC, 'hinge', 'logsumexp', 1.0, -50.0, 50.0, w_in=0.1, w_out=0.1, **kw)


def test_pretrain_step_with_roles_that_never_count_changes_nothing():
    """pre-labelled targets without a positive anchor and no outlier image: every role is -1, the regulariser adds an all-zero gradient"""
    from ood_object_detection_amd.pretrain import PretrainStep
    xs, target = _pretrain_inputs(2)
    runs = []
    for with_reg in (False, True):
        model = _model()
        step = PretrainStep(model, ood_regularizer=_hinge() if with_reg else None)
        cls_t, box_t, npos = step.targets(target)
        labelled = {'label_num_positives': npos, 'outlier': torch.tensor([False, False], device=DEV)}
        for l, (c, b) in enumerate(zip(cls_t, box_t)):
            labelled['label_cls_%d' % l] = torch.where(c >= 0, torch.full_like(c, -2), c)      # the positives become ignore labels
            labelled['label_bbox_%d' % l] = b.clone()
        outs = [step(x, labelled) for x in xs]
        if with_reg:
            for o in outs:
                assert float(o['ood_loss']) == 0.0 and int(o['n_in']) == 0 and int(o['n_out']) == 0
        else:
            assert 'ood_loss' not in outs[0]
        runs.append(([(o['loss'].item(), o['grad_norm'].item()) for o in outs],) + _state(model))
    assert runs[0][0] == runs[1][0]
    for part in (1, 2):
        for n in runs[0][part]:
            assert torch.equal(runs[0][part][n], runs[1][part][n]), n


def test_pretrain_step_adds_the_regulariser_and_replays_it_in_a_graph():
    from ood_object_detection_amd.pretrain import PretrainStep
    xs, target = _pretrain_inputs(4)
    runs = []
    for graph in (False, True):
        model = _model()
        step = PretrainStep(model, ood_regularizer=_hinge(), graph=graph, graph_warmup=2)
        hist = []
        for x in xs:
            o = step(x, target)
            assert float(o['ood_loss']) > 0.0 and int(o['n_in']) > 0 and int(o['n_out']) > 0
            assert int(o['active_in']) == int(o['n_in']) and int(o['active_out']) == int(o['n_out'])
            hist.append((o['loss'].item(), o['ood_loss'].item(), o['grad_norm'].item(), float(o['mean_energy_in']), int(o['n_out'])))
        if graph:
            assert step._cap is not None
        runs.append((hist,) + _state(model))
    assert runs[0][0] == runs[1][0], (runs[0][0], runs[1][0])
    for part in (1, 2):
        for n in runs[0][part]:
            assert torch.equal(runs[0][part][n], runs[1][part][n]), n


def test_pretrain_step_loss_is_the_detection_loss_plus_the_regulariser():
    from ood_object_detection_amd.pretrain import PretrainStep
    xs, target = _pretrain_inputs(1)
    plain = PretrainStep(_model())(xs[0], {k: v for k, v in target.items() if k != 'outlier'})
    model = _model()
    step = PretrainStep(model, ood_regularizer=_hinge())
    o = step(xs[0], target)
    assert float(o['ood_loss']) > 0.0
    assert torch.equal(o['loss'], plain['loss'] + o['ood_loss'])              # the same forward: the detection loss has the same bits
    assert torch.equal(o['class_loss'], plain['class_loss']) and torch.equal(o['box_loss'], plain['box_loss'])
    # the outlier image's anchors (also the one that carries a label) are outliers, the other image's positives in-distribution
    cls_t, _, _ = step.targets(target)
    from ood_object_detection_amd.effdet.loss import _pack_targets
    packed = _pack_targets(list(cls_t), 0)
    assert int(o['n_in']) == int((packed[0] >= 0).sum()) and int(o['n_out']) == int((packed[1] != -2).sum())
    assert float(o['grad_norm']) != float(plain['grad_norm'])
    with pytest.raises(ValueError, match='outlier'):
        step(xs[0], {k: v for k, v in target.items() if k != 'outlier'})


def test_pretrain_step_trains_phi_of_the_logistic_form():
    from ood_object_detection_amd.pretrain import PretrainStep
    xs, target = _pretrain_inputs(2)
    model = _model()
    reg = _reg(PC, 'logistic', w_in=0.1, w_out=0.1, phi=(1.0, 0.0))
    step = PretrainStep(model, ood_regularizer=reg)
    assert step.opt.params[-1] is reg.phi and len(step.opt.params) == len([p for p in model.parameters() if p.requires_grad]) + 1
    before = reg.phi.detach().clone()
    for x in xs:
        o = step(x, target)
    assert float(o['ood_loss']) > 0.0 and not torch.equal(reg.phi.detach(), before)
