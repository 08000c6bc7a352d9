"""ood_synth.OutlierSynthesizer (csrc/outlier_synth.hip) and ood_train.virtual_outlier_loss against the numpy restatement of
tests/_outlier_synth_ref.py, and their hook in pretrain.PretrainStep.

Bound of every float32 result against the float64 restatement: 4 * E32 + 1e-7 * max|value|, E32 the float32 restatement's own error
on the same inputs (`_outlier_synth_ref.bound`).  Every case prints E32, the device error and the bound before it asserts.

Cases (C, S, F, k): F 64 is one pass of 16 feature blocks, 88 a ragged one (22 blocks), 288 several; S 1, 63, 64, 65 sit around a
wave, 1000 and 10 000 are several workgroups and, at 10 000, three sort tiles; k = S keeps everything.  The seed of a case with
k < S is chosen (on the CPU, `_gaps`) so that consecutive ranks 1 .. k + 1 of the float64 r2 of every class are further apart than
twice the r2 bound: the kept set and its order are then decided, and the test asserts that on the reference before it looks at the
device.  With k = S the order must agree wherever the neighbours are that far apart, and must be r2 descending, then j ascending."""
import numpy as np
import pytest
import torch

import _outlier_synth_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DRAW = (3 << 32) | 5                                     # a draw number with both words set

#        name      C   S      F    k     seed
CASES = {
    'one':     (1, 1, 64, 1, 1),
    's63':     (3, 63, 88, 4, 1),
    's64':     (3, 64, 64, 16, 1),
    's65':     (1, 65, 288, 65, 1),
    'c90':     (90, 1000, 64, 4, 1),
    'all':     (3, 1000, 288, 1000, 1),
    'big':     (8, 10000, 88, 16, 1),
    'tiles':   (8, 4096, 288, 16, 1),
}


def _synth(F, C, S, k, seed, A=1, **kw):
    from ood_object_detection_amd.ood_synth import OutlierSynthesizer
    return OutlierSynthesizer(F, C, A, candidates=S, keep=k, seed=seed, device=DEV, **kw)


def _reference(name):
    C, S, F, k, seed = CASES[name]
    z64, z32 = R.candidates(seed, DRAW, range(C), S, F)
    r64 = np.stack([R.sqnorm(z) for z in z64])
    r32 = np.stack([R.sqnorm(z) for z in z32])
    return z64, z32, r64, r32


def _gaps(r64, k, b_r2):
    """the smallest distance between consecutive ranks 1 .. k + 1 over the classes, against 2 * bound"""
    top = -np.sort(-r64, axis=1)[:, :k + 1]
    gap = float((top[:, :-1] - top[:, 1:]).min()) if top.shape[1] > 1 else np.inf
    return gap, gap > 2.0 * b_r2


def _np(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize('name', list(CASES))
def test_sample_against_restatement(name):
    C, S, F, k, seed = CASES[name]
    z64, z32, r64, r32 = _reference(name)
    b_z = R.bound(np.abs(z32 - z64).max(), z64)
    b_r2 = R.bound(np.abs(r32 - r64).max(), r64)
    order64 = np.stack([R.select(r, S) for r in r64])

    # ---- every candidate: L = I, mu = 0, k = S gives the device's own normals and norms ---------------------------------------------
    s_all = _synth(F, C, S, S, seed).set_gaussians(np.zeros((C, F)), np.eye(F)).seek(DRAW)
    o = {key: _np(v) for key, v in s_all.sample(advance=False).items()}
    assert (np.sort(o['index'], axis=1) == np.arange(S)[None]).all()                         # a permutation of the candidates
    eps = np.empty((C, S, F), np.float32)
    r2 = np.empty((C, S), np.float32)
    for c in range(C):
        eps[c, o['index'][c]], r2[c, o['index'][c]] = o['rows'][c], o['r2'][c]
    e_z, e_r2 = np.abs(eps - z64).max(), np.abs(r2 - r64).max()
    print('%s: normals E32 %.3g device %.3g bound %.3g | r2 E32 %.3g device %.3g bound %.3g'
          % (name, np.abs(z32 - z64).max(), e_z, b_z, np.abs(r32 - r64).max(), e_r2, b_r2))
    assert e_z <= b_z and e_r2 <= b_r2
    d = np.diff(o['r2'], axis=1)
    assert (d <= 0).all() and (np.diff(o['index'], axis=1)[d == 0] > 0).all()               # r2 descending, equal r2 by j ascending
    s64 = np.take_along_axis(r64, order64, 1)
    far = np.ones((C, S), bool)                                                              # both neighbours further than 2 * bound
    far[:, 1:] &= (s64[:, :-1] - s64[:, 1:]) > 2.0 * b_r2
    far[:, :-1] &= (s64[:, :-1] - s64[:, 1:]) > 2.0 * b_r2
    assert (o['index'][far] == order64[far]).all()
    assert (o['roles'] == 0).all()
    cst = np.float32(R.log_const(np.eye(F)))
    assert np.array_equal(o['log_density'], -(o['r2'] * np.float32(0.5)) + cst)

    # ---- the kept rows with a random mean and factor --------------------------------------------------------------------------------
    mu, L = R.gaussians(F, C, seed=100 + F)
    gap, decided = _gaps(r64, k, b_r2) if k < S else (0.0, False)
    if k < S:
        print('%s: smallest gap of ranks 1 .. k + 1 %.3g against 2 * bound %.3g' % (name, gap, 2.0 * b_r2))
        assert decided, 'choose another seed for this case'
    s_k = _synth(F, C, S, k, seed).set_gaussians(mu, L).seek(DRAW)
    got = {key: _np(v) for key, v in s_k.sample(advance=False).items()}
    if k < S:
        assert np.array_equal(got['index'], order64[:, :k])                                 # the set, and the order
    assert np.array_equal(got['index'], o['index'][:, :k]) and np.array_equal(got['r2'], o['r2'][:, :k])
    idx = got['index']
    ref64 = np.stack([R.rows(mu[c], L, z64[c][idx[c]]) for c in range(C)])
    ref32 = np.stack([R.rows(mu[c], L, z32[c][idx[c]]) for c in range(C)])
    b_rows = R.bound(np.abs(ref32 - ref64).max(), ref64)
    e_rows = np.abs(got['rows'] - ref64).max()
    ld64 = -0.5 * np.take_along_axis(r64, idx, 1) + R.log_const(L)
    ld32 = -(np.take_along_axis(r32, idx, 1) * np.float32(0.5)) + np.float32(R.log_const(L))
    b_ld = R.bound(np.abs(ld32 - ld64).max(), ld64)
    e_ld = np.abs(got['log_density'] - ld64).max()
    print('%s: rows E32 %.3g device %.3g bound %.3g | log_density E32 %.3g device %.3g bound %.3g'
          % (name, np.abs(ref32 - ref64).max(), e_rows, b_rows, np.abs(ld32 - ld64).max(), e_ld, b_ld))
    assert e_rows <= b_rows and e_ld <= b_ld

    # ---- L = I: the rows are the mean plus the device's own normals, bit for bit ----------------------------------------------------
    s_i = _synth(F, C, S, k, seed).set_gaussians(mu, np.eye(F)).seek(DRAW)
    rows_i = _np(s_i.sample()['rows'])
    want = np.stack([mu[c].astype(np.float32)[None] + eps[c, idx[c]] for c in range(C)])
    assert np.array_equal(rows_i, want)
    assert s_i.draw == DRAW + 1 and s_k.draw == DRAW


def test_exact_ties_go_to_the_smaller_candidate():
    """F = 4 (through the C ABI: the Python class takes BiFPN widths only) and S = 2^16 with k = S: r2 has about 2^22 values a unit
    interval to fall on, so the draw holds equal norms, and the stable sort must keep their candidates ascending"""
    from ood_object_detection_amd import _lib
    lib = _lib.load()
    F, C, S = 4, 2, 1 << 16
    t = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=DEV)
    mu, U, cst, valid, draw = t(C, F), torch.eye(F, device=DEV), t(1), torch.ones(C, dtype=torch.int8, device=DEV), t(1, dtype=torch.int64)
    rows, index, r2, ld, roles = t(C, S, F), t(C, S, dtype=torch.int32), t(C, S), t(C, S), t(C * S, dtype=torch.int8)
    need = lib.effdet_outlier_synth_workspace_bytes(C, S)
    ws = t(need, dtype=torch.uint8)
    st = torch.cuda.current_stream(DEV).cuda_stream
    rc = lib.effdet_outlier_synth(st, F, C, C, None, S, S, 9, draw.data_ptr(), 1, mu.data_ptr(), U.data_ptr(), cst.data_ptr(), valid.data_ptr(),
                                  rows.data_ptr(), index.data_ptr(), r2.data_ptr(), ld.data_ptr(), roles.data_ptr(), ws.data_ptr(), need)
    assert rc == 0
    torch.cuda.synchronize()
    assert int(draw.item()) == 1
    r, idx, x = _np(r2), _np(index), _np(rows)
    assert (np.sort(idx, axis=1) == np.arange(S)[None]).all()
    d = np.diff(r, axis=1)
    ties = int((d == 0).sum())
    print('exact ties among 2 x %d norms: %d' % (S, ties))
    assert ties > 0 and (d <= 0).all() and (np.diff(idx, axis=1)[d == 0] > 0).all()
    z32 = np.stack([R.normals(R.words(9, 0, c, np.arange(S), F), np.float32) for c in range(C)])
    z64 = np.stack([R.normals(R.words(9, 0, c, np.arange(S), F), np.float64) for c in range(C)])
    got = np.empty_like(z32)
    for c in range(C):
        got[c, idx[c]] = x[c]
    assert np.abs(got - z64).max() <= R.bound(np.abs(z32 - z64).max(), z64)
    # out-of-range arguments: -22 before any launch
    call = lambda **kw: lib.effdet_outlier_synth(*[kw.get(n, v) for n, v in (
        ('st', st), ('F', F), ('C', C), ('n', C), ('ids', None), ('S', S), ('k', 1), ('seed', 9), ('draw', draw.data_ptr()), ('adv', 0),
        ('mu', mu.data_ptr()), ('U', U.data_ptr()), ('cst', cst.data_ptr()), ('valid', valid.data_ptr()), ('rows', rows.data_ptr()),
        ('index', index.data_ptr()), ('r2', r2.data_ptr()), ('ld', ld.data_ptr()), ('roles', roles.data_ptr()), ('ws', ws.data_ptr()),
        ('nws', need))])
    assert call() == 0
    for bad in (dict(F=6), dict(F=0), dict(F=516), dict(C=0), dict(C=1025), dict(n=0), dict(n=1025), dict(S=0), dict(S=(1 << 20) + 1),
                dict(k=0), dict(k=S + 1), dict(draw=None), dict(mu=None), dict(U=None), dict(cst=None), dict(valid=None), dict(rows=None),
                dict(index=None), dict(r2=None), dict(ld=None), dict(roles=None), dict(ws=None), dict(nws=need - 1)):
        assert call(**bad) == -22, bad
    assert lib.effdet_outlier_synth_workspace_bytes(1024, 1 << 17) == -22 and lib.effdet_outlier_synth_workspace_bytes(0, 8) == -22
    torch.cuda.synchronize()
    assert int(draw.item()) == 1


# ---- bitwise properties -------------------------------------------------------------------------------------------------------------
BC, BS, BF, BK = 20, 1000, 64, 4


def _eq(a, b):
    return all(torch.equal(a[key], b[key]) for key in ('rows', 'index', 'r2', 'log_density', 'roles'))


def _fitted(seed=4, gauss=7, valid=None, k=BK):
    mu, L = R.gaussians(BF, BC, seed=gauss)
    return _synth(BF, BC, BS, k, seed).set_gaussians(mu, L, valid)


def test_two_runs_agree_and_draws_follow_each_other():
    a, b = _fitted(), _fitted()
    a0, a1 = a.sample(), a.sample()
    b0 = b.sample()
    assert _eq(a0, b0) and not torch.equal(a0['index'], a1['index'])
    assert _eq(b.sample(), a1) and a.draw == 2
    assert not torch.equal(_fitted(seed=5).sample()['index'], a0['index'])                   # another seed, other candidates
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        a.sample(classes=torch.zeros(2, dtype=torch.int32))


def test_any_grouping_of_the_classes_gives_the_same_bits():
    a = _fitted().seek(11)
    whole = a.sample(advance=False)
    lo = a.sample(classes=range(0, 7), advance=False)
    ids = torch.tensor([19, 7, 8, 12, 9, 10, 11, 13, 14, 15, 16, 17, 18], dtype=torch.int32, device=DEV)
    hi = a.sample(classes=ids)
    assert a.draw == 12
    for key in ('rows', 'index', 'r2', 'log_density'):
        assert torch.equal(lo[key], whole[key][:7]), key
        assert torch.equal(hi[key], whole[key][ids.long()]), key
    assert torch.equal(lo['roles'], whole['roles'][:7 * BK]) and (hi['roles'] == 0).all()
    # an id outside [0, C) in a device list: an invalid class, nothing is read for it
    out = a.seek(11).sample(classes=torch.tensor([3, -1, BC, 5], dtype=torch.int32, device=DEV))
    assert torch.equal(out['rows'][0], whole['rows'][3]) and torch.equal(out['rows'][3], whole['rows'][5])
    assert not out['rows'][1:3].any() and out['roles'].view(4, BK).tolist() == [[0] * BK, [-1] * BK, [-1] * BK, [0] * BK]
    with pytest.raises(ValueError):
        a.sample(classes=[0, BC])


def test_invalid_classes_get_zero_rows_and_the_role_minus_one():
    valid = np.ones(BC, bool)
    valid[[2, 19]] = False
    full, part = _fitted().sample(), _fitted(valid=valid).sample()
    keep = torch.from_numpy(valid).to(DEV)
    assert torch.equal(part['rows'][keep], full['rows'][keep]) and not part['rows'][~keep].any() and bool(full['rows'][~keep].any())
    assert part['roles'].view(BC, BK)[keep].eq(0).all() and part['roles'].view(BC, BK)[~keep].eq(-1).all()
    for key in ('index', 'r2', 'log_density'):
        assert torch.equal(part[key], full[key]), key


def test_graph_replays_are_the_eager_draws_and_see_a_new_fit():
    a = _fitted().seek(5)
    eager = [a.sample() for _ in range(3)]
    mu2, L2 = R.gaussians(BF, BC, seed=8)
    other = _fitted(gauss=8).seek(8).sample()
    a.seek(5)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            out = a.sample()
    torch.cuda.current_stream(DEV).wait_stream(side)
    assert a.draw == 5                                                                        # capturing runs nothing
    for want in eager:
        g.replay()
        torch.cuda.synchronize()
        assert _eq(out, want)
    assert a.draw == 8
    before = out['rows'].clone()
    a.set_gaussians(mu2, L2)                                                                  # in place: the graph reads the same buffers
    g.replay()
    torch.cuda.synchronize()
    assert _eq(out, other) and not torch.equal(out['rows'], before) and a.draw == 9


def _features(seed, rows=1500, few=(0, 3)):
    """[1, rows, F] features with a class per row; class few[0] gets few[1] rows only"""
    g = np.random.default_rng(seed)
    cls = g.integers(1, BC, rows)
    cls[:few[1]] = few[0]
    x = g.standard_normal((rows, BF)) @ (np.eye(BF) + 0.1 * g.standard_normal((BF, BF))) + g.standard_normal((BC, BF))[cls]
    return torch.from_numpy(x.astype(np.float32))[None].to(DEV), torch.from_numpy(cls.astype(np.int64))[None].to(DEV)


def test_fit_from_statistics_and_state_dict_round_trip():
    from ood_object_detection_amd.ood_features import FeatureOOD
    from ood_object_detection_amd.ood_synth import gaussian_factors
    x, cls = _features(1)
    a = _synth(BF, BC, BS, BK, 4, min_count=5)
    with pytest.raises(RuntimeError, match='fit'):
        a.sample()
    with pytest.raises(ValueError):
        a.fit()                                                                               # no rows yet, like FeatureOOD.fit
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        a.add(x.cpu(), cls.cpu())
    a.add(x, cls)
    a.fit()
    p = gaussian_factors(_np(a.statistics.n_c), _np(a.statistics.s_c), _np(a.statistics.S), 0.0, 5)
    assert p['valid'].tolist() == [False] + [True] * (BC - 1)
    one = a.sample()
    assert not one['rows'][0].any() and one['roles'].view(BC, BK)[0].eq(-1).all() and one['roles'].view(BC, BK)[1:].eq(0).all()
    idx, got = _np(one['index']), _np(one['rows'])
    mu, L = p['mu'].astype(np.float32).astype(np.float64), p['L'].astype(np.float32).astype(np.float64)     # what the device holds
    for c in (1, BC - 1):
        w = R.words(4, 0, c, idx[c], BF)
        a64, a32 = R.rows(mu[c], L, R.normals(w, np.float64)), R.rows(mu[c], L, R.normals(w, np.float32))
        assert np.abs(got[c] - a64).max() <= R.bound(np.abs(a32 - a64).max(), a64)
    assert abs(float(one['log_density'][1, 0]) - (-0.5 * float(one['r2'][1, 0]) + p['log_const'])) < 1e-4
    # a shared FeatureOOD: one add pass fits both
    shared = FeatureOOD(BF, BC, 1, device=DEV)
    b = _synth(BF, BC, BS, BK, 4, min_count=5, statistics=shared)
    shared.add(x, cls)
    assert _eq(b.fit().sample(), one)
    # the state carries the seed, the draw counter and the statistics, and continues the sequence
    a.sample()
    sd = a.state_dict()
    assert sd['draw'] == 2 and sd['seed'] == 4
    nxt = a.sample()
    c = _synth(BF, BC, BS, BK, 99, min_count=1).load_state_dict(sd)
    assert c.fitted and c.seed == 4 and c.min_count == 5 and _eq(c.sample(), nxt) and c.draw == 3
    with pytest.raises(ValueError):
        _synth(BF, BC, BS, BK + 1, 4).load_state_dict(sd)
    a.clear()
    assert not a.fitted and int(a.statistics.n_c.sum()) == 0 and a.draw == 3


# ---- virtual_outlier_loss -----------------------------------------------------------------------------------------------------------
def _replica(z, role, rows, W, b, phi, w_in, w_out, dtype):
    """the loss in torch on the CPU in `dtype`: real rows with role 1 on the in side, every virtual anchor on the out side"""
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    W, b, phi = t(W).requires_grad_(), t(b).requires_grad_(), t(phi).requires_grad_()
    C = z.shape[-1]
    e_in = -torch.logsumexp(t(z).reshape(-1, C)[torch.from_numpy(role.reshape(-1) == 1)], 1)
    e_out = -torch.logsumexp((t(rows) @ W.t() + b).reshape(-1, C), 1)
    l_in = torch.nn.functional.softplus(-(phi[0] * -e_in + phi[1]))
    l_out = torch.nn.functional.softplus(phi[0] * -e_out + phi[1])
    loss = w_in * l_in.mean() + w_out * l_out.mean()
    loss.backward()
    return loss.detach().numpy(), W.grad.numpy(), b.grad.numpy(), phi.grad.numpy()


def test_virtual_outlier_loss():
    from ood_object_detection_amd.effdet import meta_ops
    from ood_object_detection_amd.ood_train import EnergyRegularizer, virtual_outlier_loss
    A, k, B, N = 9, 2, 2, 37
    w_in, w_out, phi0 = 0.75, 1.5, (0.5, -1.25)
    g = np.random.default_rng(2)
    valid = np.ones(BC, bool)
    valid[6] = False
    synth = _fitted(valid=valid, k=k)
    reg = EnergyRegularizer(BC, 'logistic', weight_in=w_in, weight_out=w_out).to(DEV)
    with torch.no_grad():
        reg.phi.copy_(torch.tensor(phi0))
    z = (2.0 * g.standard_normal((B, N, BC)) - 3.0).astype(np.float32)
    role = np.where(g.random((B, N)) < 0.4, 1, -1).astype(np.int8)
    Wn, bn = (0.1 * g.standard_normal((A * BC, BF))).astype(np.float32), g.standard_normal(A * BC).astype(np.float32)
    zt, rt = torch.from_numpy(z).to(DEV), torch.from_numpy(role).to(DEV)
    W = torch.from_numpy(Wn).to(DEV).view(A * BC, BF, 1, 1).requires_grad_()
    b = torch.from_numpy(bn).to(DEV).requires_grad_()
    s = synth.sample(advance=False)
    s['rows'].requires_grad_()
    loss, stats = virtual_outlier_loss(reg, zt, rt, synth, W, b, sample=s)
    loss.backward()
    assert s['rows'].grad is None                                                             # the sampled rows are constants
    assert synth.draw == 0
    # one call over the concatenation: the sides have separate means
    with torch.no_grad():
        v = meta_ops.Linear.apply(s['rows'].detach().view(BC * k, BF), W.detach().view(A * BC, BF), b.detach()).view(1, BC * k * A, BC)
        vr = s['roles'].view(-1, 1).expand(-1, A).reshape(1, -1)
        l_real, _ = reg(zt, rt)
        l_virt, _ = reg(v, vr)
        l_cat, st_cat = reg(torch.cat([zt.view(1, B * N, BC), v], 1), torch.cat([rt.view(1, -1), vr], 1))
    assert int(stats['n_in']) == int(st_cat['n_in']) == int((role == 1).sum()) and int(stats['n_out']) == 0
    assert int(stats['n_virtual']) == int(st_cat['n_out']) == (BC - 1) * k * A
    assert torch.equal(stats['mean_l_virtual'], st_cat['mean_l_out']) and torch.equal(stats['mean_energy_virtual'], st_cat['mean_energy_out'])
    assert torch.equal(loss.detach(), l_real + l_virt)
    # each call rounds its float64 sum to float32 once and the sum of the two is rounded again: three half-ulps of the terms
    assert abs(float(loss) - float(l_cat)) <= 3.0 * 2.0 ** -24 * (float(l_real) + float(l_virt))
    # the gradients against the float64 replica on the same rows
    rows = _np(s['rows'])[valid]
    r64 = _replica(z, role, rows, Wn, bn, phi0, w_in, w_out, torch.float64)
    r32 = _replica(z, role, rows, Wn, bn, phi0, w_in, w_out, torch.float32)
    got = (_np(loss), _np(W.grad).reshape(A * BC, BF), _np(b.grad), _np(reg.phi.grad))
    for what, x, a64, a32 in zip(('loss', 'grad weight', 'grad bias', 'grad phi'), got, r64, r32):
        e32, err = np.abs(a32 - a64).max(), np.abs(x - a64).max()
        bound = R.bound(e32, a64)
        print('virtual_outlier_loss %s: E32 %.3g device %.3g bound %.3g' % (what, e32, err, bound))
        assert err <= bound, what
    assert bool(W.grad.any()) and bool(b.grad.any())
    # by default a sample is drawn, and the next call draws the next one
    l1, _ = virtual_outlier_loss(reg, zt, rt, synth, W.detach(), b.detach())
    l2, _ = virtual_outlier_loss(reg, zt, rt, synth, W.detach(), b.detach())
    assert synth.draw == 2 and torch.equal(l1, loss.detach()) and not torch.equal(l2, l1)
    with pytest.raises(ValueError):
        virtual_outlier_loss(reg, zt, rt, synth, W.detach().view(A * BC, BF)[:, :32], b.detach())
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        virtual_outlier_loss(reg, zt, rt, synth, W.detach().cpu(), b.detach().cpu())


# ---- PretrainStep -------------------------------------------------------------------------------------------------------------------
SIZE, PB, PC, PA, PF = 128, 2, 20, 9, 64


def _pretrain_inputs(steps):
    g = torch.Generator().manual_seed(3)
    xs = [torch.randint(0, 256, (PB, 3, SIZE, SIZE), generator=g, dtype=torch.uint8).to(DEV) for _ in range(steps)]
    boxes = [torch.tensor([[10., 12., 70., 90.], [40., 30., 120., 100.]]), torch.tensor([[5., 5., 60., 50.]])]
    cls = [torch.tensor([3, 7]), torch.tensor([1])]
    return xs, {'bbox': [b.to(DEV) for b in boxes], 'cls': [c.to(DEV) for c in cls]}


def _model():
    from _models import seeded_model
    model, cfg, _, _ = seeded_model('tf_efficientdet_d0', SIZE, PC, seed=23)
    return model.to(DEV).float()


def _state(model):
    return {n: p.detach().clone() for n, p in model.named_parameters()}, {n: b.detach().clone() for n, b in model.named_buffers()}


def _logistic():
    from ood_object_detection_amd.ood_train import EnergyRegularizer
    return EnergyRegularizer(PC, 'logistic', weight_in=0.1, weight_out=0.1).to(DEV)


def _head_synth(fit, k=2):
    s = _synth(PF, PC, 1000, k, 6, A=PA)
    if fit:
        mu, L = R.gaussians(PF, PC, seed=12)
        s.set_gaussians(mu, L)
    return s


def _same_states(a, b):
    for part in (0, 1):
        for n in a[part]:
            assert torch.equal(a[part][n], b[part][n]), n


def test_pretrain_step_before_any_fit_is_the_regulariser_alone():
    from ood_object_detection_amd.effdet.loss import _pack_targets
    from ood_object_detection_amd.pretrain import PretrainStep
    xs, target = _pretrain_inputs(2)
    target = dict(target, outlier=torch.tensor([False, True], device=DEV))
    runs = []
    for with_synth in (False, True):
        model = _model()
        synth = _head_synth(False) if with_synth else None
        step = PretrainStep(model, ood_regularizer=_logistic(), outlier_synthesizer=synth, synth_refresh_every=1000)
        outs = [step(x, target) for x in xs]
        assert all('n_virtual' not in o for o in outs)
        runs.append(([(o['loss'].item(), o['ood_loss'].item(), o['grad_norm'].item()) for o in outs],) + _state(model))
        if with_synth:
            cls_t, _, _ = step.targets(target)
            packed = _pack_targets(list(cls_t), 0)
            want = torch.bincount(packed[packed >= 0].reshape(-1), minlength=PC) * 2           # every positive anchor, both steps
            assert torch.equal(synth.statistics.n_c, want) and int(want.sum()) > 0 and not synth.fitted and synth.draw == 0
    assert runs[0][0] == runs[1][0]
    _same_states(runs[0][1:], runs[1][1:])
    with pytest.raises(ValueError, match='ood_regularizer'):
        PretrainStep(_model(), outlier_synthesizer=_head_synth(False))
    with pytest.raises(ValueError):
        PretrainStep(_model(), ood_regularizer=_logistic(), outlier_synthesizer=_synth(PF, PC + 1, 1000, 2, 6, A=PA))


def test_pretrain_step_adds_the_virtual_outliers_after_a_fit():
    from ood_object_detection_amd.effdet import meta_ops
    from ood_object_detection_amd.pretrain import PretrainStep
    xs, target = _pretrain_inputs(1)                                                          # no target['outlier']: optional with a synthesiser
    plain = PretrainStep(_model())(xs[0], target)
    alone_model = _model()
    alone = PretrainStep(alone_model, ood_regularizer=_logistic())(xs[0], dict(target, outlier=torch.tensor([False, False], device=DEV)))
    model, synth = _model(), _head_synth(True)
    step = PretrainStep(model, ood_regularizer=_logistic(), outlier_synthesizer=synth, synth_refresh_every=1000)
    o = step(xs[0], target)
    assert float(o['ood_loss']) > 0.0 and int(o['n_virtual']) == PC * 2 * PA and int(o['n_out']) == 0 and int(o['n_in']) == int(alone['n_in'])
    assert torch.equal(o['loss'], plain['loss'] + o['ood_loss'])                              # the same forward: the same detection loss
    assert torch.equal(o['class_loss'], plain['class_loss']) and torch.equal(o['box_loss'], plain['box_loss'])
    assert float(o['ood_loss']) > float(alone['ood_loss']) and synth.draw == 1
    g_with, g_alone = model.class_net.predict.conv_pw.weight.grad, alone_model.class_net.predict.conv_pw.weight.grad
    assert not torch.equal(g_with, g_alone)
    assert torch.equal(model.class_net.conv_rep[0].conv_pw.weight.grad, alone_model.class_net.conv_rep[0].conv_pw.weight.grad)   # real side only

    # the accessor: per-level [B, F, h, w], the depthwise conv of the tower output, of which the logits are an affine map
    m2 = _model()
    PretrainStep(m2, ood_regularizer=_logistic(), outlier_synthesizer=_head_synth(True))(xs[0], target)
    eng = m2._train_engine
    class_out, _ = m2(m2(xs[0], mode='bb'), mode='fpn_and_head')                              # a training forward on the engine
    pen, tower = eng.class_penultimate(), eng.class_penultimate(tower=True)
    head = m2.class_net.predict
    taps = head.conv_dw.weight.detach().reshape(PF, 9).t().contiguous()
    Wp, bias = head.conv_pw.weight.detach().reshape(PA * PC, PF), head.conv_pw.bias.detach()
    assert len(pen) == len(class_out) == 5
    for lvl, (p, t, z) in enumerate(zip(pen, tower, class_out)):
        assert p.shape[:2] == (PB, PF) and p.shape[2:] == z.shape[2:] and p.stride(1) == 1 and not p.requires_grad
        x = t.permute(0, 2, 3, 1).contiguous()
        dw = meta_ops.DwConv.apply(x, taps)
        b_dw = 17 * 2.0 ** -23 * float(taps.abs().sum(0).max()) * float(x.abs().max())        # nine products and eight sums, two orders
        e_dw = float((dw - p.permute(0, 2, 3, 1)).abs().max())
        logits = p.permute(0, 2, 3, 1).double() @ Wp.double().t() + bias.double()
        b_pw = PF * 2.0 ** -23 * float(Wp.abs().sum(1).max()) * float(p.abs().max())          # a float32 dot product of F terms
        e_pw = float((logits - z.detach().permute(0, 2, 3, 1).double()).abs().max())
        print('level %d: depthwise error %.3g bound %.3g | logits error %.3g bound %.3g' % (lvl, e_dw, b_dw, e_pw, b_pw))
        assert e_dw <= b_dw and e_pw <= b_pw


def test_pretrain_step_with_a_synthesiser_replays_in_a_graph():
    from ood_object_detection_amd.pretrain import PretrainStep
    xs, target = _pretrain_inputs(4)
    runs = []
    for graph in (False, True):
        model, synth = _model(), _head_synth(True)
        step = PretrainStep(model, ood_regularizer=_logistic(), outlier_synthesizer=synth, synth_refresh_every=3, synth_shrinkage=0.5,
                            graph=graph, graph_warmup=2)
        hist = []
        for i, x in enumerate(xs):
            o = step(x, target)
            assert int(o['n_virtual']) > 0
            hist.append((o['loss'].item(), o['ood_loss'].item(), o['grad_norm'].item(), int(o['n_virtual']), float(o['mean_energy_virtual'])))
            assert (synth.shrinkage == 0.5) == (i >= 2)                                       # the fit from the statistics, after step 3
        if graph:
            assert step._cap is not None
        assert synth.draw == 4
        runs.append((hist, _state(model), synth.state_dict()))
    assert runs[0][0] == runs[1][0], (runs[0][0], runs[1][0])
    _same_states(runs[0][1], runs[1][1])
    for key in ('n_c', 's_c', 'S'):
        assert torch.equal(runs[0][2]['statistics'][key], runs[1][2]['statistics'][key]), key
    assert runs[0][0][3][3] < PC * 2 * PA                                                     # the new fit: classes without rows are not valid
