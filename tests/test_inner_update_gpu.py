"""episode.inner_update (csrc/inner_update.hip) against the torch composition of infer.py:660-678, `par - par_lr * inner_grad`.

Forward and d g are compared with torch.equal: the kernels round the product and the difference separately, as torch does, so the
float32 CPU composition gives the same bits.  d p is the cotangent.  d lr_k is a sum of exact float64 products taken in float64 and
rounded once; against the same sum taken by torch in float64 in another order the only differences are float64 rounding and the one
final rounding, so it must be float32(reference) or one of its two float32 neighbours.  The second-order chain and the end-to-end
step use the yardsticks of tests/test_support_loss_gpu.py."""
import functools

import pytest
import torch

import _inner_update_ref as iref

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'

# ---- list 1: every size class of the kernel in one launch.  1, 3, 9: below one vector / a tail after two vectors; 576: vectors only;
# 1023 / 1025: a tail of 3 / 1 floats; 4096: two full workgroups; 82944 (the 288 x 288 pointwise weight): 41 workgroups, the last one
# ragged.  conv_pw2 is a view 4 bytes into its storage (scalar path), conv_dw0 / conv_pw0 / conv_pb0 share step size 0, step size 3
# is used by nothing, step size 1 does not require grad, conv_pb2's gradient is None, bn_w00 passes through.
LIST1 = [('conv_dw0', (64, 1, 3, 3)), ('conv_pw0', (288, 288, 1, 1)), ('conv_pb0', (1,)), ('conv_pb1', (3,)), ('conv_dw2', (1023,)),
         ('conv_pw2', (1025,)), ('conv_pb2', (7,)), ('predict_dw', (4096,)), ('predict_pb', (9,)), ('bn_w00', (64,))]
LIST1_LR = [0.11, 0.07, 0.23, 0.5, 0.031, 0.9]
LIST1_NONE = ('conv_pb2',)
# ---- list 3: 40 updated tensors, more than one launch takes; step sizes 0 .. 4 each span both launches
LIST3 = [('extra_w%d_%02d' % (i % 5, i), (1 + (37 * i) % 701,)) for i in range(40)]
LIST3_LR = [0.3, 0.05, 0.11, 0.17, 0.021]


def _lists():
    return {'list1': (LIST1, LIST1_LR, LIST1_NONE, ('conv_pw2',)),
            'd0': (iref.meta_head_shapes(64, 3), [0.05, 0.075, 0.1, 0.125, 0.15], (), ()),
            'd5_sep': (iref.meta_head_shapes(288, 4, add_head=True), [0.05, 0.07, 0.09, 0.11, 0.13, 0.15], (), ()),
            'list3': (LIST3, LIST3_LR, (), ())}


@functools.lru_cache(maxsize=None)
def _case(key, separate_head=False):
    """CPU side of a case, computed once: tensors, the plan, the float32 composition and its gradients, the float64 d lr"""
    from ood_object_detection_amd.episode import plan_inner_update
    named_shapes, lr_vals, none_names, offset = _lists()[key]
    ps, gs, Ws = iref.seeded_list(len(named_shapes), named_shapes, offset)
    names = [n for n, _ in named_shapes]
    gs = [None if n in none_names else g for n, g in zip(names, gs)]
    plan = plan_inner_update(names, len(lr_vals), False, separate_head)
    lrs = [torch.tensor(v) for v in lr_vals]
    fast = iref.literal_update(list(zip(names, ps)), gs, lrs, False, separate_head, skip_none=True)
    d_g = [None if (k is None or g is None) else (-W) * lrs[k] for W, g, k in zip(Ws, gs, plan)]
    d_lr = iref.lr_grad_f64(Ws, gs, plan, len(lr_vals))
    return dict(names=names, ps=ps, gs=gs, Ws=Ws, plan=plan, lr_vals=lr_vals, fast=fast, d_g=d_g, d_lr=d_lr, offset=offset,
                separate_head=separate_head)


def _to_dev(t, offset_view=False):
    if t is None:
        return None
    if offset_view:                                            # keep the 4-byte offset into a storage of its own
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
        buf[1:].copy_(t.reshape(-1))
        v = buf[1:].reshape(t.shape)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v
    return t.to(DEV, copy=True)


def _device_case(case, frozen=()):
    """-> params (leaves), grads (leaves requiring grad, so that d g is observable), cotangents, step sizes"""
    ps = [_to_dev(p, n in case['offset']).requires_grad_() for n, p in zip(case['names'], case['ps'])]
    gs = [None if g is None else _to_dev(g, n in case['offset']).requires_grad_() for n, g in zip(case['names'], case['gs'])]
    Ws = [_to_dev(W, n in case['offset']) for n, W in zip(case['names'], case['Ws'])]
    lrs = [torch.tensor(v, device=DEV, requires_grad=k not in frozen) for k, v in enumerate(case['lr_vals'])]
    return ps, gs, Ws, lrs


def _run(case, frozen=()):
    from ood_object_detection_amd import episode
    ps, gs, Ws, lrs = _device_case(case, frozen)
    fast = episode.inner_update(zip(case['names'], ps), gs, lrs, separate_head=case['separate_head'])
    outer = sum((f * W).sum() for f, W in zip(fast, Ws))
    live_g = [g for g in gs if g is not None]
    live_lr = [l for l in lrs if l.requires_grad]
    grads = torch.autograd.grad(outer, ps + live_g + live_lr, allow_unused=True)
    n = len(ps)
    it_g, it_lr = iter(grads[n:n + len(live_g)]), iter(grads[n + len(live_g):])
    d_g = [None if g is None else next(it_g) for g in gs]
    d_lr = [next(it_lr) if l.requires_grad else None for l in lrs]
    return dict(ps=ps, gs=gs, Ws=Ws, lrs=lrs, fast=fast, d_p=list(grads[:n]), d_g=d_g, d_lr=d_lr)


def _neighbours(x64):
    """float32(x) and its two float32 neighbours"""
    r = torch.tensor(x64, dtype=torch.float64).to(torch.float32)
    return [float(torch.nextafter(r, torch.tensor(-float('inf')))), float(r), float(torch.nextafter(r, torch.tensor(float('inf'))))]


def _check_lr_grads(got, case, frozen=(), factor=1.0):
    for k, (g, want) in enumerate(zip(got, case['d_lr'])):
        if want is None or k in frozen:
            assert g is None, ('step size', k)
            continue
        assert g is not None and g.shape == (), ('step size', k)
        ok = _neighbours(want * factor)
        print('d lr[%d]: device %.9g, float32(float64 sum) %.9g' % (k, float(g), ok[1]))
        assert float(g) in ok, ('step size', k, float(g), ok)


@pytest.mark.parametrize('key,separate_head', [('list1', False), ('d0', False), ('d5_sep', False), ('d5_sep', True), ('list3', False)])
def test_forward_and_first_order(key, separate_head):
    from ood_object_detection_amd import _lib
    case = _case(key, separate_head)
    frozen = (1,)
    out = _run(case, frozen)
    updated = sum(1 for k, g in zip(case['plan'], case['gs']) if k is not None and g is not None)
    if key == 'list3':
        assert updated > _lib.load().effdet_inner_update_max_tensors()
    if key == 'list1':
        assert sorted(int(p.numel()) for p, k, g in zip(case['ps'], case['plan'], case['gs']) if k is not None and g is not None) == \
            [1, 3, 9, 576, 1023, 1025, 4096, 82944]
        assert case['plan'].count(0) == 3 and 3 not in case['plan']
    assert len(out['fast']) == len(case['names'])
    for n, k, p, g, f, want, d_p, d_g, want_dg, W in zip(case['names'], case['plan'], out['ps'], out['gs'], out['fast'], case['fast'],
                                                         out['d_p'], out['d_g'], case['d_g'], out['Ws']):
        if k is None or g is None:
            assert f is p, n                                    # passes through as the same object
            assert torch.equal(d_p, W), n
            assert d_g is None or not bool(d_g.any()), n
            continue
        assert f is not p and f.shape == p.shape and f.dtype == torch.float32, n
        assert torch.equal(f.detach().cpu(), want), n           # p - lr * g with torch's two roundings
        assert torch.equal(d_p, W), n                           # d p is the cotangent
        assert torch.equal(d_g.cpu(), want_dg), n               # (-G) * lr
    _check_lr_grads(out['d_lr'], case, frozen)
    if separate_head:
        assert out['fast'][case['names'].index('predict_pw')] is out['ps'][case['names'].index('predict_pw')]
        assert out['fast'][case['names'].index('predict_pw_sep')] is not out['ps'][case['names'].index('predict_pw_sep')]


def test_python_float_step_sizes_and_no_lr_gradient():
    """Python numbers travel by value and get no gradient; when no step size wants one, d g and d p still arrive"""
    from ood_object_detection_amd import episode
    case = _case('list1')
    ps, gs, Ws, _ = _device_case(case)
    fast = episode.inner_update(zip(case['names'], ps), gs, list(case['lr_vals']))
    for n, f, want in zip(case['names'], fast, case['fast']):
        assert torch.equal(f.detach().cpu(), want), n
    live = [(g, W, w) for g, W, w in zip(gs, Ws, case['d_g']) if w is not None]
    d_g = torch.autograd.grad(sum((f * W).sum() for f, W in zip(fast, Ws)), [g for g, _, _ in live])
    for got, (_, _, want) in zip(d_g, live):
        assert torch.equal(got.cpu(), want)
    # a 1-element (not 0-d) step size tensor: same bits, gradient in its own shape
    ps, gs, Ws, lrs = _device_case(case)
    lrs[0] = torch.tensor([case['lr_vals'][0]], device=DEV, requires_grad=True)
    fast = episode.inner_update(zip(case['names'], ps), gs, lrs)
    assert torch.equal(fast[0].detach().cpu(), case['fast'][0])
    d0, = torch.autograd.grad(sum((f * W).sum() for f, W in zip(fast, Ws)), [lrs[0]])
    assert d0.shape == (1,) and float(d0) in _neighbours(case['d_lr'][0])


def test_lr_grad_accumulates_over_backward_calls():
    from ood_object_detection_amd import episode
    case = _case('list1')
    ps, gs, Ws, lrs = _device_case(case)
    fast = episode.inner_update(zip(case['names'], ps), gs, lrs)
    outer = sum((f * W).sum() for f, W in zip(fast, Ws))
    once = torch.autograd.grad(outer, [lrs[0], lrs[2]], retain_graph=True)
    outer.backward(retain_graph=True)
    assert lrs[3].grad is None                                  # used by nothing
    first = [lrs[0].grad.clone(), lrs[2].grad.clone()]
    assert all(torch.equal(a, b) for a, b in zip(first, once))
    (2 * outer).backward()
    for k, f in zip((0, 2), first):
        assert torch.equal(lrs[k].grad, f + 2 * f)              # doubling the cotangent is exact, .grad adds in float32
    assert torch.equal(ps[0].grad, 3 * Ws[0])


def test_non_contiguous_gradients_and_non_leaf_parameters():
    from ood_object_detection_amd import episode
    gen = torch.Generator().manual_seed(3)
    base = torch.randn(48, 20, generator=gen)
    g_t = torch.randn(20, 48, generator=gen)
    W = torch.randn(48, 20, generator=gen)
    lr = torch.tensor(0.3)
    p_dev = base.to(DEV).requires_grad_()
    p_nonleaf = p_dev * 1.0                                     # an earlier fast weight
    g_dev = g_t.to(DEV).requires_grad_()
    lr_dev = lr.to(DEV).requires_grad_()
    fast, = episode.inner_update([('conv_dw0', p_nonleaf)], (g_dev.t(),), [lr_dev, 0.0])
    assert torch.equal(fast.detach().cpu(), base - lr * g_t.t())
    # a non-contiguous cotangent as well
    outer = (fast.t() * W.t().contiguous().to(DEV)).sum()
    d_p, d_g, d_lr = torch.autograd.grad(outer, [p_dev, g_dev, lr_dev])
    assert torch.equal(d_p.cpu(), W) and torch.equal(d_g.cpu(), ((-W) * lr).t())
    assert float(d_lr) in _neighbours(-float((W.double() * g_t.t().double()).sum()))


# ---- second-order chain ---------------------------------------------------------------------------------------------------------

CHAIN_SHAPES = [(1,), (9,), (5, 205), (64, 1, 3, 3), (4096,)]
CHAIN_NAMES = ['conv_pb0', 'conv_pb1', 'conv_pw1', 'predict_dw', 'predict_pw']
CHAIN_LR = [0.2, 0.11, 0.05, 0.3, 0.07]                         # step size 2 is used by nothing


def _chain_inputs():
    gen = torch.Generator().manual_seed(21)
    mk = lambda: [torch.randn(s, generator=gen) for s in CHAIN_SHAPES]
    return dict(base=mk(), coef=mk(), cubic=mk(), square=mk(), q=mk(), r=mk(), u=torch.randn(len(CHAIN_SHAPES), generator=gen))


def _chain(dtype, device, update):
    """p_t = base_t + coef_t u_t with an upstream leaf u (so p_t is not a leaf); inner loss sum_t mean(cubic_t p_t^3 + square_t p_t^2) (products spelled out),
    differentiated with create_graph; fast weights; outer loss sum_t mean(q_t fast_t^2 + r_t fast_t).  -> the outer loss's gradients
    with respect to p (concatenated), the step sizes that are used, and u."""
    c = {k: ([t.to(device=device, dtype=dtype) for t in v] if isinstance(v, list) else v.to(device=device, dtype=dtype)) for k, v in _chain_inputs().items()}
    u = c['u'].clone().requires_grad_()
    lrs = [torch.tensor(v, dtype=dtype, device=device, requires_grad=True) for v in CHAIN_LR]
    ps = [b + k * u[i] for i, (b, k) in enumerate(zip(c['base'], c['coef']))]
    inner = sum((a * p * p * p + s * p * p).mean() for a, s, p in zip(c['cubic'], c['square'], ps))
    inner_grad = torch.autograd.grad(inner, ps, create_graph=True)
    fast = update(list(zip(CHAIN_NAMES, ps)), inner_grad, lrs)
    outer = sum((q * f * f + r * f).mean() for q, r, f in zip(c['q'], c['r'], fast))
    used = [k for k in range(len(lrs)) if k != 2]
    grads = torch.autograd.grad(outer, ps + [lrs[k] for k in used] + [u])
    n = len(ps)
    return {'p': torch.cat([g.reshape(-1) for g in grads[:n]]).detach().cpu().double(),
            'lr': torch.stack(list(grads[n:-1])).detach().cpu().double(), 'u': grads[-1].detach().cpu().double()}


def test_second_order_chain():
    """the same program in float64 on the CPU is the reference; E32 is the error of that program in float32 on the CPU; the device
    (inner_update for the update, torch for the rest) must be within 4 E32 + 1e-7 of the largest entry, per gradient"""
    from ood_object_detection_amd import episode
    literal = lambda named, grad, lrs: iref.literal_update(named, grad, lrs)
    want = _chain(torch.float64, 'cpu', literal)
    want32 = _chain(torch.float32, 'cpu', literal)
    got = _chain(torch.float32, DEV, episode.inner_update)
    for key in ('p', 'lr', 'u'):
        scale = float(want[key].abs().max())
        e32 = float((want32[key] - want[key]).abs().max())
        err = float((got[key] - want[key]).abs().max())
        print('second-order chain, d %s: E32 %.3e, device error %.3e, largest entry %.3e' % (key, e32, err, scale))
        assert scale > 0 and bool(torch.isfinite(got[key]).all())
        assert err <= 4 * e32 + 1e-7 * scale, (key, err, e32, scale)


# ---- repeatability --------------------------------------------------------------------------------------------------------------

def _flat(out):
    return [t.detach().clone() for t in out['fast']] + [t.clone() for t in out['d_g'] if t is not None] + \
        [t.clone() for t in out['d_lr'] if t is not None]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('key', ['list1', 'list3'])
def test_two_calls_give_the_same_bits(key):
    case = _case(key)
    assert _same(_flat(_run(case)), _flat(_run(case)))


def test_graph_capture_reads_step_sizes_on_the_device():
    from ood_object_detection_amd import episode
    case = _case('list1')
    ps, gs, Ws, lrs = _device_case(case)

    def step():
        fast = episode.inner_update(zip(case['names'], ps), gs, lrs)
        outer = sum((f * W).sum() for f, W in zip(fast, Ws))
        used = [l for k, l in enumerate(lrs) if k != 3]
        grads = torch.autograd.grad(outer, [g for g, k in zip(gs, case['plan']) if g is not None and k is not None] + used)
        return [f.detach() for f in fast] + list(grads)

    def set_lrs(scale):
        with torch.no_grad():
            for l, v in zip(lrs, case['lr_vals']):
                l.fill_(v * scale)

    eager1 = [t.clone() for t in step()]
    set_lrs(1.5)
    eager2 = [t.clone() for t in step()]
    assert not torch.equal(eager1[0], eager2[0])
    set_lrs(1.0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for scale, eager in ((1.0, eager1), (1.5, eager2), (1.0, eager1)):
        set_lrs(scale)                                          # in place: the captured launches keep their arguments
        graph.replay()
        torch.cuda.synchronize()
        assert _same(captured, eager), scale


# ---- argument checks ------------------------------------------------------------------------------------------------------------

def test_unsupported_arguments_raise():
    from ood_object_detection_amd import episode
    p = torch.zeros(8, device=DEV)
    g = torch.ones(8, device=DEV)
    lr = torch.tensor(0.1, device=DEV)
    with pytest.raises(RuntimeError, match='on the GPU'):
        episode.inner_update([('conv_dw0', p)], [g], [torch.nn.Parameter(torch.tensor(0.1)), lr])       # infer.py:244-250 as written
    with pytest.raises(RuntimeError, match='float32'):
        episode.inner_update([('conv_dw0', p.bfloat16())], [g.bfloat16()], [lr, lr])
    with pytest.raises(RuntimeError, match='float32'):
        episode.inner_update([('conv_dw0', p)], [g], [lr.double(), lr])
    with pytest.raises(ValueError, match='shape'):
        episode.inner_update([('conv_dw0', p)], [torch.ones(2, 4, device=DEV)], [lr, lr])
    with pytest.raises(ValueError, match='conv_dw2'):
        episode.inner_update([('conv_dw2', p)], [g], [lr, lr])                                         # learnable_lr[2] of two
    with pytest.raises(RuntimeError, match='GPU'):
        episode.inner_update([('conv_dw0', p)], [g.cpu()], [lr, lr])
    with pytest.raises(ValueError, match='empty'):
        episode.inner_update([('conv_dw0', p[:0])], [g[:0]], [lr, lr])
    with pytest.raises(ValueError, match='step sizes'):
        episode.inner_update([('conv_dw0', p)], [g], [lr] * 17)


# ---- end to end -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('steps', [1, 2])
def test_end_to_end_meta_phase_step_with_learnable_lr(golden, steps):
    """tests/test_support_loss_gpu.py::test_end_to_end_meta_phase_step with episode.inner_update and layers + 2 distinct learnable step
    sizes, for one and for two inner steps (the second step's parameters are the first step's fast weights), against the CPU replica
    through the oracle with the literal loop.  The step sizes' gradients are compared as well, within 1e-3 of their largest entry."""
    import _episode_ref as ref
    import _support_loss_ref as sref
    import test_infer_proj_gpu as tip
    from oracle import model as om
    from ood_object_detection_amd import episode
    from ood_object_detection_amd.effdet.config import get_efficientdet_config
    from ood_object_detection_amd.effdet.efficientdet import MetaHead, ProjectionNet
    OFFSET = tip.OFFSET
    names = dict(get_efficientdet_config=get_efficientdet_config, MetaHead=MetaHead, ProjectionNet=ProjectionNet)
    c, mh, proj_net, mh_names, ref_params, proj_ref, dots_ref = tip._setup(names, golden)
    B, n_lr = c['B'], c['R'] + 2
    lr_vals = [0.05 + 0.1 * k / (n_lr - 1) for k in range(n_lr)]              # 0.05 ... 0.15
    lrs_gpu = [torch.nn.Parameter(torch.tensor(v, device=DEV)) for v in lr_vals]
    lrs_cpu = [torch.nn.Parameter(torch.tensor(v)) for v in lr_vals]
    gen = torch.Generator().manual_seed(17)
    qry_x = [torch.randn(t.shape, generator=gen) for t in c['x']]
    qry_w = [torch.randn(B, tip.NUM_ANCHS, s, s, generator=gen) for s in c['sizes'][OFFSET:]]

    def outer(params, head, update, lrs, first_loss, supp_loss_of, xs, xq):
        """the inner steps, then the weighted query sum of the original test"""
        fast, loss = params, first_loss
        for s in range(steps):
            if s > 0:
                loss = supp_loss_of(*head(fast, xs))
            inner_grad = torch.autograd.grad(loss, fast, allow_unused=True, create_graph=True)
            fast = update(list(zip(mh_names, fast)), inner_grad, lrs)
        qry_out = head(fast, xq)[0]
        return sum((o * w.to(o.device)).sum() for o, w in zip(qry_out, qry_w)) / B

    params = list(mh.parameters())

    def head_gpu(ps, x):
        if ps is params:
            return mh(x, ret_activs=True, level_offset=OFFSET)
        return mh(x, fast_weights=ps, ret_activs=True, level_offset=OFFSET)

    xs_gpu = [t.clone().to(DEV) for t in c['x']]
    confs, activs = head_gpu(params, xs_gpu)
    picked = episode.select_anchors(confs)
    feed, conf = episode.projection_feed(activs, confs, picked, proj_net, first_level=OFFSET)
    gather = lambda outs: torch.cat([cl.movedim(1, 3).reshape(B, -1).gather(1, s.long()) for cl, s in zip(outs, picked)], dim=1).reshape(-1)
    logits = gather(confs)
    assert torch.equal(logits.detach(), conf.reshape(-1))
    proj_embds = proj_net(feed)
    proj_embds = proj_embds.reshape(-1, proj_embds.shape[-1])
    dm, da = proj_net.dot_mult, proj_net.dot_add
    sel = episode.cluster(proj_embds, conf.reshape(-1), B, dm, da)
    assert int(sel['n_valid']) > 0

    def supp_gpu(outs, _activs):
        lg = gather(outs)
        return episode.support_loss(proj_embds, lg, lg, sel, dm, da)['loss']

    supp = supp_gpu(confs, activs)
    loss = outer(params, head_gpu, episode.inner_update, lrs_gpu, supp, supp_gpu, xs_gpu, [t.to(DEV) for t in qry_x])
    loss.backward()
    proj_params = [m.weight for m in proj_net.projection if isinstance(m, torch.nn.Linear)]
    # ---- CPU replica
    head_cpu = lambda ps, x: tip._oracle_head(c, mh_names, ps, x)
    xs_cpu = [t.clone() for t in c['x']]
    outs_r, activs_r = head_cpu(ref_params, xs_cpu)
    masks = [torch.zeros(B, o.shape[1] * o.shape[2] * o.shape[3], dtype=torch.bool).scatter_(1, s.cpu().long(), True)
             for o, s in zip(outs_r, picked)]
    enc = [t.cpu() for t in (proj_net.anch_enc, proj_net.lev_enc, proj_net.cell_enc)]
    feed_r, _, _ = ref.episode_feed(activs_r, outs_r, *enc, first_level=OFFSET, masks=masks)
    embds_r = om.projection_forward(proj_ref, feed_r.detach().reshape(-1, feed_r.shape[-1]))
    sel_cpu = {k: sel[k].cpu() for k in ('proto0', 'valid', 'proto', 'nearest')}

    def supp_cpu(outs, activs_):
        lg = ref.episode_feed(activs_, outs, *enc, first_level=OFFSET, masks=masks)[1].reshape(-1)
        return sref.loss_literal(embds_r, lg, lg, sel_cpu, dots_ref[0], dots_ref[1], B)[0]

    supp_r = supp_cpu(outs_r, activs_r)
    literal = lambda named, grad, lrs: iref.literal_update(named, grad, lrs, skip_none=True)
    loss_r = outer(ref_params, head_cpu, literal, lrs_cpu, supp_r, supp_cpu, xs_cpu, qry_x)
    print('steps %d: support loss %.6g, replica %.6g; query loss %.6g, replica %.6g' % (steps, float(supp.detach()), float(supp_r.detach()), float(loss.detach()), float(loss_r.detach())))
    assert abs(float(supp.detach()) - float(supp_r.detach())) <= 1e-3 * abs(float(supp_r.detach()))
    assert abs(float(loss.detach()) - float(loss_r.detach())) <= 1e-3 * max(1e-3, abs(float(loss_r.detach())))
    gr = torch.autograd.grad(loss_r, proj_ref + ref_params + lrs_cpu, allow_unused=True)
    n_proj, n_par = len(proj_params), len(ref_params)
    for p in proj_params:
        assert p.grad is not None and float(p.grad.abs().max()) > 0
    tip._compare([p.grad for p in proj_params], gr[:n_proj], 1e-3, 'proj_net')
    used = [(p.grad, r_) for p, r_ in zip(mh.parameters(), gr[n_proj:n_proj + n_par]) if r_ is not None]
    tip._compare([g for g, _ in used], [r_ for _, r_ in used], 1e-3, 'class_net')
    lr_ref = gr[n_proj + n_par:]
    assert all(r_ is not None for r_ in lr_ref) and all(l.grad is not None for l in lrs_gpu)
    print('step-size gradients: device %s, replica %s' % ([float(l.grad) for l in lrs_gpu], [float(r_) for r_ in lr_ref]))
    tip._compare([l.grad for l in lrs_gpu], lr_ref, 1e-3, 'learnable_lr')
