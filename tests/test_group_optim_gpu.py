"""optim.GroupedOptimizer (csrc/group_optim.hip) against torch's own optimizers and clip_grad_norm_, run on the CPU in float64 on
identical parameter and gradient values (tests/_group_optim_ref.py).

Bound for parameters and state after every step: 4 E32 + 1e-7 max(1, |ref|max), E32 being the deviation of torch's float32 run
from its float64 run on the same case (test_group_optim_host.py prints it): the device rounds like the float32 run, up to another
association of a few operations.  Per-domain norms: 1e-5 max(1, norm) (the bound of test_flat_adam_matches_oracle).
"""
import numpy as np
import pytest
import torch

import _group_optim_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
QUANT = ('params', 'state1', 'state2')


def _dev(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float32)).to(DEV)


def _build(optim, p0=None, groups=None, domains=None, hyper=None):
    """-> (params in SHAPES order, optimizer); groups / domains hold index lists like the reference driver's"""
    from ood_object_detection_amd.optim import GroupedOptimizer
    p0 = R.scenario_data()[0] if p0 is None else p0
    params = [torch.nn.Parameter(_dev(a)) for a in p0]
    groups = R.scenario_groups() if groups is None else groups
    domains = R.scenario_domains() if domains is None else domains
    tg = [dict(g, params=[params[i] for i in g['params']]) for g in groups]
    td = [dict(d, params=[params[i] for i in d['params']]) for d in domains]
    opt = GroupedOptimizer(tg, optim=optim, clip_domains=td, **(R.HYPER[optim] if hyper is None else hyper))
    return params, opt


def _feed(opt, params, row):
    """zero_grad, then the step's gradients by in-place adds into p.grad (a pair (a, b): two adds); a parameter without one gets
    junk in its slot, which must not matter.  -> the present parameters"""
    opt.zero_grad()
    present = []
    for p, g in zip(params, row):
        if g is None:
            if p.grad is not None:
                p.grad.fill_(1e3)
            continue
        for part in (g if isinstance(g, tuple) else (g,)):
            if part is not None:
                p.grad.add_(_dev(part))
        present.append(p)
    return present


def _snapshot(opt, params, norms=None):
    idx = [opt._index[id(p)] for p in params]
    steps = opt._step.cpu().tolist()
    snap = {'params': [p.detach().cpu().numpy().copy() for p in params],
            'state1': [opt._view(opt.state1, i).cpu().numpy().copy() for i in idx],
            'state2': [(opt._view(opt.state2, i).cpu().numpy().copy() if opt.state2 is not None else np.zeros(tuple(p.shape), np.float32))
                       for i, p in zip(idx, params)],
            'steps': [steps[opt._seg_of[i]] for i in idx]}
    if norms is not None:
        snap['norms'] = norms.cpu().tolist()
    return snap


def _check_buffers(opt, params):
    """every parameter and gradient at a 64-byte address; all padding of every flat buffer zero"""
    pad = torch.ones(opt.flat_param.numel(), dtype=torch.bool, device=DEV)
    for i, p in enumerate(opt.params):
        off = opt.layout['offsets'][i]
        pad[off:off + p.numel()] = False
        assert p.data_ptr() % 64 == 0 and p.data_ptr() == opt.flat_param.data_ptr() + 4 * off
        if p.grad is not None:
            assert p.grad.data_ptr() == opt.flat_grad.data_ptr() + 4 * off
    assert int(pad.sum()) == opt.flat_param.numel() - sum(p.numel() for p in opt.params)
    for flat in (opt.flat_param, opt.flat_grad, opt.state1, opt.state2):
        if flat is not None:
            assert not bool(flat[pad].any())


def _run_scenario(optim, check=True):
    p0, grads = R.scenario_data()
    params, opt = _build(optim)
    snaps = []
    for k in range(R.STEPS):
        if k + 1 == R.LR_EDIT_STEP:
            opt.param_groups[R.LR_EDIT_GROUP]['lr'] = R.LR_EDIT_VALUE
        present = _feed(opt, params, grads[k])
        norms = opt.step(present=present)
        snaps.append(_snapshot(opt, params, norms))
        if check:
            _check_buffers(opt, params)
    return snaps


def _equal(a, b):
    return all(np.array_equal(x, y) for q in QUANT for s, t in zip(a, b) for x, y in zip(s[q], t[q])) and \
        all(s['steps'] == t['steps'] and s.get('norms') == t.get('norms') for s, t in zip(a, b))


def _compare(snaps, ref, e, what, tensors=None):
    """every step, every quantity within 4 E32 + 1e-7 max(1, |ref|max); prints the largest deviation per quantity"""
    worst = dict.fromkeys(QUANT, 0.0)
    for k, (s, r) in enumerate(zip(snaps, ref)):
        for q in QUANT:
            sel = range(len(s[q])) if tensors is None else tensors
            err = max(float(np.abs(s[q][i].astype(np.float64) - r[q][i]).max()) for i in sel)
            worst[q] = max(worst[q], err)
            lim = R.bound(e[q], [r[q][i] for i in sel])
            print('%s step %d %s: deviation %.3e, E32 %.3e, bound %.3e' % (what, k + 1, q, err, e[q], lim))
            assert err <= lim, (what, k + 1, q, err, lim)
    print('%s largest deviations: %s' % (what, ', '.join('%s %.3e' % (q, worst[q]) for q in QUANT)))
    return worst


@pytest.mark.parametrize('optim', ['adam', 'sgd'])
def test_six_step_scenario_matches_torch(optim):
    ref, e = R.scenario_pair(optim)
    assert ref[1]['coefs'][0] == 1.0 and ref[1]['coefs'][1] < 1.0            # exactly one domain clips in step 2
    p0, _ = R.scenario_data()
    snaps = _run_scenario(optim)
    _compare(snaps, ref, e, optim)
    for k, (s, r) in enumerate(zip(snaps, ref)):
        for got, want in zip(s['norms'], r['norms']):
            print('%s step %d norm: %.8e, torch %.8e, relative %.2e' % (optim, k + 1, got, want, abs(got - want) / max(1.0, want)))
            assert abs(got - want) <= 1e-5 * max(1.0, want)
        assert s['steps'] == r['steps']                                      # Adam: per-parameter count; SGD: a buffer exists
        for i in (R.NEVER, R.NORM_ONLY):                                     # never updated / norm only: not a bit of it moves
            assert np.array_equal(s['params'][i], np.asarray(p0[i])) and not s['state1'][i].any() and not s['state2'][i].any()
    assert len(snaps[0]['norms']) == 2


@pytest.mark.parametrize('optim', ['adam', 'sgd'])
def test_two_runs_give_the_same_bits(optim):
    assert _equal(_run_scenario(optim, check=False), _run_scenario(optim, check=False))


def test_same_work_as_flat_adam():
    """one group, one domain, all present: the work of FlatAdam"""
    from ood_object_detection_amd.optim import FlatAdam
    rs = np.random.RandomState(77)
    p0 = [rs.normal(0, 1, s).astype(np.float32) for s in R.SHAPES]
    rows = [[(rs.normal(0, 1, s) * sc).astype(np.float32) for s in R.SHAPES] for sc in (1e-3, 0.5, 1e-3)]     # step 2 clips
    n = len(p0)
    groups, domains = [{'params': list(range(n))}], [{'params': list(range(n)), 'max_norm': 10.0}]
    hyper = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    ref = R.run_reference('adam', p0, rows, groups, domains, torch.float64, hyper=hyper)[0]
    e = R.deviation(R.run_reference('adam', p0, rows, groups, domains, torch.float32, hyper=hyper)[0], ref)
    assert ref[1]['coefs'][0] < 1.0
    params, opt = _build('adam', p0, groups, domains, hyper=hyper)
    fparams = [torch.nn.Parameter(_dev(a)) for a in p0]
    flat = FlatAdam(fparams, lr=1e-3, max_grad_norm=10.0)
    snaps = []
    for row in rows:
        _feed(opt, params, row)
        norms = opt.step()
        _feed(flat, fparams, row)
        fnorm = float(flat.step())
        snaps.append(_snapshot(opt, params, norms))
        assert abs(snaps[-1]['norms'][0] - fnorm) <= 1e-5 * max(1.0, fnorm)
    _compare(snaps, ref, e, 'flat-adam work')
    _check_buffers(opt, params)


@pytest.mark.parametrize('optim', ['adam', 'sgd'])
def test_layout_does_not_matter(optim):
    """reversed order, another grouping, same hyper-parameters, no clipping: the update is elementwise"""
    p0, grads = R.scenario_data()
    n = len(p0)
    rows = [[None if g is None else R.summed(g) for g in row] for row in grads[2:5]]
    a_params, a = _build(optim, groups=[{'params': [i for i in range(n) if i % 3 == g]} for g in range(3)], domains=[])
    b_params, b = _build(optim, groups=[{'params': list(range(n - 1, 4, -1))}, {'params': list(range(4, -1, -1))}], domains=[])
    assert a.layout['offsets'] != b.layout['offsets']
    for row in rows:
        na = a.step(present=_feed(a, a_params, row))
        nb = b.step(present=_feed(b, b_params, row))
        assert na.numel() == 0 and nb.numel() == 0
    sa, sb = _snapshot(a, a_params), _snapshot(b, b_params)
    assert _equal([sa], [sb])
    assert not np.array_equal(sa['params'][0], np.asarray(p0[0]))


def _graph_rows():
    """five steps whose present set changes from step to step (tensor 3 misses step 1, 4 misses 2, 5 misses 4; NEVER all)"""
    _, grads = R.scenario_data()
    rows = [[None if g is None else R.summed(g) for g in row] for row in grads[:5]]
    rows[3][5] = None
    return rows


@pytest.mark.parametrize('optim', ['adam', 'sgd'])
def test_captured_step_equals_eager(optim):
    rows = _graph_rows()
    e_params, eager = _build(optim)
    g_params, opt = _build(optim)
    for k, row in enumerate(rows):
        if k + 1 == R.LR_EDIT_STEP:
            eager.param_groups[R.LR_EDIT_GROUP]['lr'] = R.LR_EDIT_VALUE
        eager.step(present=_feed(eager, e_params, row))
    for row in rows[:2]:
        opt.step(present=_feed(opt, g_params, row))
    before = _snapshot(opt, g_params)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        norms = opt.step()                                                   # records the launches; nothing runs, nothing is uploaded
    assert _equal([_snapshot(opt, g_params)], [before])
    for k in range(2, 5):
        if k + 1 == R.LR_EDIT_STEP:
            opt.param_groups[R.LR_EDIT_GROUP]['lr'] = R.LR_EDIT_VALUE
        opt.set_present(_feed(opt, g_params, rows[k]))                      # gradients go into the static flat_grad
        assert opt.refresh() is True                                         # something changed every time here
        assert opt.refresh() is False
        graph.replay()
    torch.cuda.synchronize()
    assert norms.shape == (2,)
    assert _equal([_snapshot(opt, g_params)], [_snapshot(eager, e_params)])
    # step counts advanced on the device: tensor 0 (index 0) took 5 steps, tensor 3 (index 1) and tensor 5 (index 10) four
    sd = opt.state_dict()
    assert 3 not in sd['state']                                              # R.NEVER is index 3 of group 0
    if optim == 'adam':
        assert [float(sd['state'][j]['step']) for j in (0, 1, 10)] == [5.0, 4.0, 4.0]
    else:
        assert all('momentum_buffer' in sd['state'][j] for j in (0, 1, 10))


def _torch_step(tparams, topt, row, domains):
    for p, g in zip(tparams, row):
        p.grad = None if g is None else torch.from_numpy(np.asarray(g)).to(p.dtype).clone()
    for d in domains:
        torch.nn.utils.clip_grad_norm_([tparams[i] for i in d['params']], d['max_norm'], foreach=False)
    topt.step()


@pytest.mark.parametrize('optim', ['adam', 'sgd'])
def test_state_dict_round_trips_with_torch(optim):
    p0, grads = R.scenario_data()
    rows = [[None if g is None else R.summed(g) for g in row] for row in grads[:4]]
    groups, domains, e = R.scenario_groups(), R.scenario_domains(), R.e32(optim)
    cls = torch.optim.Adam if optim == 'adam' else torch.optim.SGD
    # device -> torch: three device steps, export, one more step on both sides
    params, opt = _build(optim)
    for row in rows[:3]:
        opt.step(present=_feed(opt, params, row))
    sd = opt.state_dict()
    assert set(sd['state']) == set(range(13)) - {3}                          # 13 grouped parameters; index 3 (R.NEVER) never updated
    assert [g['params'] for g in sd['param_groups']] == [list(range(0, 5)), list(range(5, 9)), list(range(9, 13))]
    tparams = [torch.nn.Parameter(p.detach().cpu().clone()) for p in params]
    topt = cls([dict(g, params=[tparams[i] for i in g['params']]) for g in groups], foreach=False, **R.HYPER[optim])
    topt.load_state_dict(sd)
    assert topt.param_groups[1]['lr'] == 0.0 and topt.param_groups[2]['weight_decay'] == 0.1
    opt.param_groups[1]['lr'] = topt.param_groups[1]['lr'] = R.LR_EDIT_VALUE
    opt.step(present=_feed(opt, params, rows[3]))
    _torch_step(tparams, topt, rows[3], domains)
    for i, (p, t) in enumerate(zip(params, tparams)):
        err = float((p.detach().cpu().double() - t.detach().double()).abs().max())
        assert err <= R.bound(e['params'], [t.detach().numpy()]), (i, err)
    back = opt.state_dict()
    for j, st in topt.state_dict()['state'].items():
        for key, q in (('exp_avg', 'state1'), ('exp_avg_sq', 'state2'), ('momentum_buffer', 'state1')):
            if key in st:
                err = float((back['state'][j][key].cpu().double() - st[key].double()).abs().max())
                assert err <= R.bound(e[q], [st[key].numpy()]), (j, key, err)
        if optim == 'adam':
            assert float(back['state'][j]['step']) == float(st['step'])
    assert set(back['state']) == set(topt.state_dict()['state'])
    # torch -> device: three torch steps in float32, its state loaded here, one more step on both sides
    _, topt, tparams = R.run_reference(optim, p0, rows[:3], groups, domains, torch.float32)
    tsd = topt.state_dict()
    assert 3 not in tsd['state'] or not tsd['state'][3]                      # no momentum buffer / moments yet
    params, opt = _build(optim, p0=[p.detach().numpy() for p in tparams])
    opt.load_state_dict(tsd)
    opt.param_groups[1]['lr'] = topt.param_groups[1]['lr'] = R.LR_EDIT_VALUE
    opt.step(present=_feed(opt, params, rows[3]))
    _torch_step(tparams, topt, rows[3], domains)
    snap = _snapshot(opt, params)
    for i, t in enumerate(tparams):
        err = float(np.abs(snap['params'][i].astype(np.float64) - t.detach().double().numpy()).max())
        assert err <= R.bound(e['params'], [t.detach().numpy()]), (i, err)
    assert not np.array_equal(snap['params'][1], np.asarray(p0[1]))          # group 1 moves once its lr is set
    want = [int(topt.state[t]['step']) if optim == 'adam' and topt.state.get(t) else (1 if topt.state.get(t, {}).get('momentum_buffer') is not None else 0)
            for t in tparams]
    assert snap['steps'] == want
    _check_buffers(opt, params)


def test_refusals_leave_a_valid_optimizer_alone():
    from ood_object_detection_amd.optim import GroupedOptimizer
    _, grads = R.scenario_data()
    rows = [[None if g is None else R.summed(g) for g in row] for row in grads[:2]]
    a_params, a = _build('adam')
    b_params, b = _build('adam')
    for k, row in enumerate(rows):
        a.step(present=_feed(a, a_params, row))
        ptrs = [p.data_ptr() for p in b_params]
        with pytest.raises(RuntimeError):
            GroupedOptimizer([{'params': [b_params[1], torch.nn.Parameter(torch.zeros(4))]}])                        # a CPU parameter
        with pytest.raises(RuntimeError):
            GroupedOptimizer([{'params': [b_params[1], torch.nn.Parameter(torch.zeros(4, dtype=torch.bfloat16, device=DEV))]}])
        with pytest.raises(ValueError):
            GroupedOptimizer([{'params': b_params[:3]}, {'params': b_params[2:4]}])                                 # in two groups
        with pytest.raises(NotImplementedError):
            GroupedOptimizer([{'params': b_params}], amsgrad=True)
        with pytest.raises(NotImplementedError):
            GroupedOptimizer([{'params': b_params}], optim='sgd', momentum=0.9, dampening=0.1)
        assert [p.data_ptr() for p in b_params] == ptrs
        b.step(present=_feed(b, b_params, row))
    assert _equal([_snapshot(a, a_params)], [_snapshot(b, b_params)])


def test_pretrain_step_with_script_groups():
    """PretrainStep(optimizer=...) with the groups of pretrain.py:184-185 (BiFPN at lr 0, backbone in no group, one clip over the
    whole model): d0, 256 px, 2 images, two eager iterations.  Backbone and BiFPN keep their bits; the heads follow
    torch.optim.Adam run on the CPU on the gradients the step saw."""
    from _models import seeded_model
    from ood_object_detection_amd.optim import GroupedOptimizer, script_param_groups
    from ood_object_detection_amd.pretrain import PretrainStep
    model = seeded_model('tf_efficientdet_d0', 256, 20, seed=11)[0].to(DEV).float()
    groups, domains = script_param_groups(model, meta_lr=1e-3)
    opt = GroupedOptimizer(groups, optim='adam', lr=1e-3, clip_domains=domains)
    assert [g['lr'] for g in opt.param_groups] == [0., 1e-3, 1e-3]
    step = PretrainStep(model, optimizer=opt)
    assert step.opt is opt
    p0 = [p.detach().cpu().numpy().copy() for p in opt.params]
    seen, inner = [], opt.step

    def spy(*a, **k):
        seen.append(opt.flat_grad.clone())
        return inner(*a, **k)
    opt.step = spy
    g = torch.Generator().manual_seed(3)
    target = {'bbox': [torch.tensor([[20., 24., 140., 180.], [80., 60., 240., 200.]]).to(DEV), torch.tensor([[10., 10., 120., 100.]]).to(DEV)],
              'cls': [torch.tensor([3, 7]).to(DEV), torch.tensor([1]).to(DEV)]}
    norms = []
    for _ in range(2):
        x = torch.randint(0, 256, (2, 3, 256, 256), generator=g, dtype=torch.uint8).to(DEV)
        out = step(x, target)
        assert out['grad_norm'].shape == (1,)
        norms.append(float(out['grad_norm'][0]))
    assert len(seen) == 2
    rows = [[opt._view(flat, i).cpu().numpy().copy() for i in range(len(opt.params))] for flat in seen]
    igroups = [dict({k: v for k, v in g.items() if k != 'params'}, params=[opt._index[id(p)] for p in g['params']]) for g in groups]
    idomains = [{'params': [opt._index[id(p)] for p in domains[0]['params']], 'max_norm': domains[0]['max_norm']}]
    hyper = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    ref = R.run_reference('adam', p0, rows, igroups, idomains, torch.float64, hyper=hyper)[0]
    e = R.deviation(R.run_reference('adam', p0, rows, igroups, idomains, torch.float32, hyper=hyper)[0], ref)
    heads = igroups[1]['params'] + igroups[2]['params']
    still = [i for i in range(len(opt.params)) if i not in set(heads)]
    assert len(still) > 100 and len(heads) > 20
    snap = _snapshot(opt, opt.params)
    _compare([snap], [ref[-1]], e, 'pretrain step heads', tensors=heads)
    for i in still:                                                          # BiFPN (lr 0) and backbone (no group)
        assert np.array_equal(snap['params'][i], p0[i]), i
    moved = max(float(np.abs(snap['params'][i] - p0[i]).max()) for i in heads)
    assert moved > 1e-4
    for got, r in zip(norms, ref):
        assert abs(got - r['norms'][0]) <= 1e-5 * max(1.0, r['norms'][0])
    backbone = {id(p) for p in model.backbone.parameters()}
    for i, p in enumerate(opt.params):                                       # the backbone is in no group: no state, no step
        if id(p) in backbone:
            assert snap['steps'][i] == 0 and not snap['state1'][i].any()
