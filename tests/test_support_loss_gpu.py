"""episode.support_loss (csrc/episode_support.hip) at its three orders against the float64 lean form of tests/_support_loss_ref.py,
which tests/test_support_loss_host.py shows equal to the literal n x n form of infer.py:607-656.

Inputs.  Rows from _episode_ref.clustered_rows, confs ~ N(0, 1) with dot_mult 1.5, dot_add 0.25, class logits ~ N(0, 2), an
upstream g in [0.5, 1.5), cotangents ~ N(0, 1).  The decisions are the float64 cluster_lean ones, uploaded, so nothing depends on
float32 argmax ties (one image alone has no valid prototype by the rule of infer.py:438; its prototype is then declared valid).

Bounds.  Values: 2e-5 of max|ref|.  First order: 1e-4 of the largest entry of that gradient in the float64 form.  Second order:
E32 is the error of the same lean form evaluated in float32 on the CPU and differentiated twice by torch, measured per output against
float64; the device must be within 4 E32 + 1e-7 x the largest entry (another summation order through three nested reductions; a
dropped or mis-signed term is an O(1) relative error)."""
import functools
import types

import pytest
import torch

import _episode_ref as ref
import _support_loss_ref as sref
from _episode_cases import DEV, OFFSET, _device_sel, _levels, _same

pytestmark = pytest.mark.gpu

ALL = (0, 1, 2, 3, 4)
# num, rows, d, seed
SHAPES = [(1, 7, 40, 1),           # m = 1, d below one wave
          (3, 50, 200, 2),         # d not a multiple of 64
          (25, 252, 256, 2),       # the meta-phase default
          (64, 5, 256, 4),         # m d = 16384 exactly
          (4, 33, 512, 5),         # largest d
          (25, 340, 64, 7)]        # n = 8500 > 32 x 256: a part holds more than 256 rows, the last part and block are ragged
SECOND_SHAPES = [SHAPES[0], SHAPES[1], SHAPES[2], SHAPES[5]]
_ids = lambda s: '%dx%d-d%d' % s[:3] if isinstance(s, tuple) and len(s) == 4 else str(s)


@functools.lru_cache(maxsize=None)
def _case(shape, sim_target, saturated=False):
    num, rows, d, seed = shape
    case = sref.draw(seed, num, rows, d, sim_target, saturated)
    if int(case['sel']['valid'].sum()) == 0:
        assert num == 1
        case['sel'] = dict(case['sel'], valid=torch.ones_like(case['sel']['valid']))
    return case


@functools.lru_cache(maxsize=None)
def _ref(shape, sim_target, dtype, thresh_grad=True, shared_head=False, present=ALL, saturated=False):
    return sref.orders(_case(shape, sim_target, saturated), 'lean', dtype, sim_target, thresh_grad, shared_head, present)


def _gpu(case, sim_target='max', thresh_grad=True, shared_head=False, present=ALL, second=True, sel=None):
    from ood_object_detection_amd import episode
    leaves = [case['x'].to(DEV, copy=True).requires_grad_(), case['confs'].to(DEV, copy=True).requires_grad_(),
              case['logits'].to(DEV, copy=True).requires_grad_(), torch.tensor(case['dm'], device=DEV, requires_grad=True),
              torch.tensor(case['da'], device=DEV, requires_grad=True)]
    g = torch.tensor(case['g'], device=DEV, requires_grad=True)
    logits = leaves[1] if shared_head else leaves[2]
    res = episode.support_loss(leaves[0], leaves[1], logits, _device_sel(case['sel'] if sel is None else sel), leaves[3], leaves[4],
                               sim_target, thresh_grad)
    assert res['loss'].dim() == 0 and not res['target'].requires_grad
    grads = torch.autograd.grad(res['loss'], leaves, grad_outputs=g, create_graph=second, allow_unused=True)
    out = dict(loss=res['loss'].detach(), target=res['target'], grads=[None if t is None else t.detach() for t in grads])
    if second:
        scalar = sum((grads[i] * case['V'][i].to(DEV)).sum() for i in present if grads[i] is not None)
        hv = torch.autograd.grad(scalar, [g] + leaves, allow_unused=True)
        out.update(d_g=hv[0], hvp=list(hv[1:]))
    return out


def _cpu(t):
    return t.detach().cpu().double()


def _close(got, want, what, bound=2e-5):
    want = want.double()
    scale = float(want.abs().max())
    err = float((_cpu(got) - want).abs().max())
    print('%s: max err %.3e, max|ref| %.3e' % (what, err, scale))
    assert err <= bound * scale, (what, err, scale)


def _check_first(got, want, what, thresh_grad=True, shared_head=False):
    for i, name in enumerate(sref.NAMES):
        w = want['grads'][i]
        if w is None:
            none_ok = (i == 2 and shared_head) or (i in (1, 3, 4) and not thresh_grad)
            assert none_ok and (got['grads'][i] is None or float(got['grads'][i].abs().max()) == 0.), (what, name)
            continue
        assert got['grads'][i] is not None and bool(torch.isfinite(got['grads'][i]).all()), (what, name)
        _close(got['grads'][i], w, '%s d %s' % (what, name), 1e-4)


def _check_second(got, want, want32, what):
    """-> the (E32, device error) pairs relative to the largest entry, for the figures DESIGN.md quotes"""
    figures = []
    for name, g, w, w32 in [('d g', got['d_g'], want['d_g'], want32['d_g'])] + \
            [('hvp ' + n, got['hvp'][i], want['hvp'][i], want32['hvp'][i]) for i, n in enumerate(sref.NAMES)]:
        if w is None:
            assert g is None or float(g.abs().max()) == 0., (what, name)
            continue
        assert g is not None and bool(torch.isfinite(g).all()), (what, name)
        scale = float(w.abs().max())
        e32 = float((w32.double() - w).abs().max())
        err = float((_cpu(g) - w).abs().max())
        print('%s %s: E32 %.3e, device error %.3e, largest entry %.3e' % (what, name, e32, err, scale))
        figures.append((name, e32, err, scale))
    for name, e32, err, scale in figures:
        assert err <= 4 * e32 + 1e-7 * scale, (what, name, err, e32, scale)
    return figures


# ---- 1. values ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('sim_target', ['max', 'avg'])
@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_values(shape, sim_target):
    from ood_object_detection_amd import episode
    case = _case(shape, sim_target)
    want = _ref(shape, sim_target, torch.float64)
    got = _gpu(case, sim_target, second=False)
    _close(got['loss'], want['loss'], 'loss')
    _close(got['target'], want['target'], 'target')
    # on cluster's own decisions: its target
    x, confs, logits = (case[k].to(DEV) for k in ('x', 'confs', 'logits'))
    out = episode.cluster(x, confs, shape[0], case['dm'], case['da'], valid_threshold=-1. if shape[0] == 1 else None, sim_target=sim_target)
    own = episode.support_loss(x, confs, logits, out, case['dm'], case['da'], sim_target)
    assert bool(torch.isfinite(out['target']).all())
    _close(own['target'], out['target'].cpu(), "cluster's target")


# ---- 2. first order -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('sim_target', ['max', 'avg'])
@pytest.mark.parametrize('shape', SHAPES, ids=_ids)
def test_first_order(shape, sim_target):
    got = _gpu(_case(shape, sim_target), sim_target, second=False)
    _check_first(got, _ref(shape, sim_target, torch.float64), '%s %s' % (_ids(shape), sim_target))


@pytest.mark.parametrize('sim_target', ['max', 'avg'])
def test_first_order_with_a_shared_head(sim_target):
    shape = SHAPES[1]
    got = _gpu(_case(shape, sim_target), sim_target, shared_head=True, second=False)
    _check_first(got, _ref(shape, sim_target, torch.float64, shared_head=True), 'confs is cls_logits', shared_head=True)


@pytest.mark.parametrize('sim_target', ['max', 'avg'])
def test_first_order_with_a_constant_threshold(sim_target):
    shape = SHAPES[1]
    got = _gpu(_case(shape, sim_target), sim_target, thresh_grad=False, second=False)
    assert all(got['grads'][i] is None or float(got['grads'][i].abs().max()) == 0. for i in (1, 3, 4))
    _check_first(got, _ref(shape, sim_target, torch.float64, thresh_grad=False), 'thresh_grad=False', thresh_grad=False)


def test_a_row_that_is_prototype_first_prototype_and_an_ordinary_row():
    shape = SHAPES[1]
    case = _case(shape, 'max')
    sel = {k: v.clone() for k, v in case['sel'].items()}
    r = 50 + 17                                                     # a row of image 1
    sel['proto'][1] = r
    sel['proto0'][1] = r
    sel['valid'][1] = True
    sel['nearest'][r] = 0                                           # and an ordinary row of prototype 0
    twisted = dict(case, sel=sel)
    want = sref.orders(twisted, 'lean', torch.float64)
    want32 = sref.orders(twisted, 'lean', torch.float32)
    got = _gpu(twisted)
    _close(got['loss'], want['loss'], 'loss')
    _check_first(got, want, 'one row, three roles')
    _check_second(got, want, want32, 'one row, three roles')


# ---- 3. second order ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('present', [ALL, (2,), (0,)], ids=['all', 'only-V_x', 'only-V_e'])
@pytest.mark.parametrize('sim_target', ['max', 'avg'])
@pytest.mark.parametrize('shape', SECOND_SHAPES, ids=_ids)
def test_second_order(shape, sim_target, present):
    got = _gpu(_case(shape, sim_target), sim_target, present=present)
    what = '%s %s %s' % (_ids(shape), sim_target, present)
    _check_second(got, _ref(shape, sim_target, torch.float64, present=present), _ref(shape, sim_target, torch.float32, present=present), what)


@pytest.mark.parametrize('sim_target', ['max', 'avg'])
def test_second_order_with_a_constant_threshold_and_a_shared_head(sim_target):
    shape = SHAPES[1]
    for kw in (dict(thresh_grad=False), dict(shared_head=True), dict(thresh_grad=False, shared_head=True)):
        got = _gpu(_case(shape, sim_target), sim_target, **kw)
        _check_second(got, _ref(shape, sim_target, torch.float64, **kw), _ref(shape, sim_target, torch.float32, **kw), str(kw))


# ---- 4. saturated logits and confidences ----------------------------------------------------------------------------------------

@pytest.mark.parametrize('sim_target', ['max', 'avg'])
@pytest.mark.parametrize('shape', SHAPES[1:3], ids=_ids)
def test_saturated_logits_and_confidences(shape, sim_target):
    case = _case(shape, sim_target, True)
    assert float((case['dm'] * (case['confs'] + case['da'])).abs().min()) > 39 and float(case['logits'].abs().min()) == 40
    want = _ref(shape, sim_target, torch.float64, saturated=True)
    got = _gpu(case, sim_target)
    assert bool(torch.isfinite(got['loss'])) and bool(torch.isfinite(got['target']).all())
    _close(got['loss'], want['loss'], 'loss')
    _close(got['target'], want['target'], 'target')
    _check_first(got, want, 'saturated')
    _check_second(got, want, _ref(shape, sim_target, torch.float32, saturated=True), 'saturated')


# ---- 5. empty valid set ---------------------------------------------------------------------------------------------------------

def test_empty_valid_set_gives_nan_everywhere_and_stays_in_range():
    shape = SHAPES[1]
    case = _case(shape, 'max')
    empty = dict(case['sel'], valid=torch.zeros_like(case['sel']['valid']))
    got = _gpu(case, sel=empty)
    torch.cuda.synchronize()
    assert bool(torch.isnan(got['loss'])) and bool(torch.isnan(got['target']).all())
    for i, name in enumerate(sref.NAMES):
        assert bool(torch.isnan(got['grads'][i]).all()), name
    assert bool(torch.isnan(got['hvp'][0]).all()) and bool(torch.isnan(got['hvp'][2]).all()) and bool(torch.isnan(got['d_g']))


def test_avg_does_not_read_the_valid_set():
    """infer.py:650-652 never touches target_clust: with no valid prototype everything stays finite and equals the float64 form"""
    shape = SHAPES[1]
    avg = _case(shape, 'avg')
    none_valid = dict(avg, sel=dict(avg['sel'], valid=torch.zeros_like(avg['sel']['valid'])))
    want, want32 = sref.orders(none_valid, 'lean', torch.float64, 'avg'), sref.orders(none_valid, 'lean', torch.float32, 'avg')
    got = _gpu(none_valid, 'avg')
    _close(got['loss'], want['loss'], "'avg' loss with an empty valid set")
    _close(got['target'], want['target'], "'avg' target with an empty valid set")
    _close(want['loss'], _ref(shape, 'avg', torch.float64)['loss'], 'the yardstick does not read it either', 1e-15)
    _check_first(got, want, "'avg', empty valid set")
    _check_second(got, want, want32, "'avg', empty valid set")


# ---- 6. repeats -----------------------------------------------------------------------------------------------------------------

def _flat(out):
    return [out['loss'], out['target'], out['d_g']] + [t for t in out['grads'] + out['hvp'] if t is not None]


@pytest.mark.parametrize('sim_target', ['max', 'avg'])
def test_two_calls_of_all_three_passes_give_the_same_bits(sim_target):
    case = _case(SHAPES[2], sim_target)
    first, again = _flat(_gpu(case, sim_target)), _flat(_gpu(case, sim_target))
    assert len(first) == 13 and all(torch.equal(a, b) for a, b in zip(first, again))
    # numbers instead of device tensors for dot_mult / dot_add: the same bits
    from ood_object_detection_amd import episode
    x, confs, logits = (case[k].to(DEV).requires_grad_() for k in ('x', 'confs', 'logits'))
    res = episode.support_loss(x, confs, logits, _device_sel(case['sel']), case['dm'], case['da'], sim_target)
    grads = torch.autograd.grad(res['loss'], [x, confs, logits], grad_outputs=torch.tensor(case['g'], device=DEV))
    assert torch.equal(res['loss'], first[0]) and all(torch.equal(a, b) for a, b in zip(grads, first[3:6]))


# ---- 7. graph capture -----------------------------------------------------------------------------------------------------------

def test_chain_with_all_three_passes_in_one_graph_replays_bit_for_bit():
    from ood_object_detection_amd import episode
    from ood_object_detection_amd.effdet.efficientdet import ProjectionNet
    B, Fc, sides = 5, 64, [16, 8, 4]
    torch.manual_seed(3)
    proj_net = ProjectionNet(types.SimpleNamespace(fpn_channels=Fc), 128).to(DEV)
    rows = sum(episode.kept_per_level(s, s) for s in sides)
    gen = torch.Generator().manual_seed(5)
    w_e, w_x = torch.randn(B * rows, 64, generator=gen).to(DEV), torch.randn(B * rows, generator=gen).to(DEV)

    def chain(activs, confs):
        with torch.no_grad():
            sel = episode.select_anchors(confs)
            feed, conf = episode.projection_feed(activs, confs, sel, proj_net, first_level=OFFSET)
            embds = proj_net(feed).reshape(-1, 64)
            out = episode.cluster(embds, conf.reshape(-1), B, proj_net.dot_mult, proj_net.dot_add)
        embds = embds.detach().requires_grad_()
        logits = conf.reshape(-1).detach().requires_grad_()                  # one head: the class logits are the confidences
        dm, da = proj_net.dot_mult.detach().requires_grad_(), proj_net.dot_add.detach().requires_grad_()
        res = episode.support_loss(embds, logits, logits, out, dm, da)
        inner = torch.autograd.grad(res['loss'], [embds, logits], create_graph=True)
        scalar = (inner[0] * w_e).sum() + (inner[1] * w_x).sum()
        return [res['loss'].detach(), res['target']] + [t.detach() for t in inner] + list(torch.autograd.grad(scalar, [embds, logits, dm, da]))

    a1, c1 = _levels(31, B, Fc, sides)
    a2, c2 = _levels(32, B, Fc, sides)
    static_a = [t.clone(memory_format=torch.preserve_format) for t in a1]
    static_c = [t.clone(memory_format=torch.preserve_format) for t in c1]
    eager1 = [t.clone() for t in chain(a1, c1)]
    eager2 = [t.clone() for t in chain(a2, c2)]
    assert bool(torch.isfinite(eager1[0])) and float(eager1[4].abs().max()) > 0 and not torch.equal(eager1[4], eager2[4])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain(static_a, static_c)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = chain(static_a, static_c)
    for (na, nc), eager in (((a2, c2), eager2), ((a1, c1), eager1)):
        for s, t in zip(static_a, na):
            s.copy_(t)
        for s, t in zip(static_c, nc):
            s.copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        assert _same(captured, eager)


# ---- 8. memory ------------------------------------------------------------------------------------------------------------------

def test_no_n_by_n_buffer_at_any_order():
    from ood_object_detection_amd import episode
    shape = SHAPES[5]
    case = _case(shape, 'max')
    x, confs, logits = (case[k].to(DEV).requires_grad_() for k in ('x', 'confs', 'logits'))
    sel = _device_sel(case['sel'])
    v_e, v_x = case['V'][0].to(DEV), case['V'][2].to(DEV)

    def step(x, confs, logits, sel, v_e, v_x):
        res = episode.support_loss(x, confs, logits, sel, case['dm'], case['da'])
        inner = torch.autograd.grad(res['loss'], [x, logits], create_graph=True)
        scalar = (inner[0] * v_e).sum() + (inner[1] * v_x).sum()
        return res, inner, torch.autograd.grad(scalar, [x, confs, logits])

    k = 4 * shape[0]
    small = dict(proto0=torch.arange(shape[0], device=DEV), proto=torch.arange(shape[0], device=DEV), valid=sel['valid'], nearest=sel['nearest'][:k])
    step(x[:k], confs[:k], logits[:k], small, v_e[:k], v_x[:k])                # library loaded, allocator warm
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    res, inner, hv = step(x, confs, logits, sel, v_e, v_x)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    input_bytes = (x.numel() + confs.numel() + logits.numel()) * 4
    print('peak memory grew by %d bytes across loss + gradient + second order, inputs are %d bytes (%.2f x)' % (grown, input_bytes, grown / input_bytes))
    assert grown < 4 * input_bytes                                  # one n x n float32 matrix would be 130 x the inputs
    want = _ref(shape, 'max', torch.float64)
    _close(res['loss'], want['loss'], 'loss')
    assert bool(torch.isfinite(hv[0]).all())


# ---- 9. end to end --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('stop_grad', [False, True])
def test_end_to_end_meta_phase_step(golden, stop_grad):
    """tests/test_infer_proj_gpu.py::test_meta_phase_outer_gradient_reaches_proj_net with the episode stage on the device: the seeded
    MetaHead, select_anchors / projection_feed / proj_net / cluster, support_loss, the create_graph=True inner gradient (infer.py:658),
    fast weights (:660-678), the query pass (:681-683) and the outer backward (:687) - against a CPU replica through the oracle that is
    given the GPU's decisions.  The feed is a copy without history; stop_grad detaches the embeddings in the inner loss as well
    (FLAGS.proj_stop_grad), and proj_net then gets no gradient."""
    import test_infer_proj_gpu as tip
    from oracle import model as om
    from ood_object_detection_amd import episode
    from ood_object_detection_amd.effdet.config import get_efficientdet_config
    from ood_object_detection_amd.effdet.efficientdet import MetaHead, ProjectionNet
    names = dict(get_efficientdet_config=get_efficientdet_config, MetaHead=MetaHead, ProjectionNet=ProjectionNet)
    c, mh, proj_net, mh_names, ref_params, proj_ref, dots_ref = tip._setup(names, golden)
    inner_lr, B = 0.1, c['B']
    gen = torch.Generator().manual_seed(17)
    qry_x = [torch.randn(t.shape, generator=gen) for t in c['x']]
    qry_w = [torch.randn(B, tip.NUM_ANCHS, s, s, generator=gen) for s in c['sizes'][OFFSET:]]

    def outer(params, head, supp_class_loss, xq):
        inner_grad = torch.autograd.grad(supp_class_loss, params, allow_unused=True, create_graph=True)
        fast = [p if (g is None or n.startswith('bn_')) else p - inner_lr * g for n, p, g in zip(mh_names, params, inner_grad)]
        qry_out = head(fast, xq)[0]
        return sum((o * w.to(o.device)).sum() for o, w in zip(qry_out, qry_w)) / B

    params = list(mh.parameters())

    def head_gpu(ps, x):
        if ps is params:
            return mh(x, ret_activs=True, level_offset=OFFSET)
        return mh(x, fast_weights=ps, ret_activs=True, level_offset=OFFSET)

    confs, activs = head_gpu(params, [t.clone().to(DEV) for t in c['x']])
    picked = episode.select_anchors(confs)
    feed, conf = episode.projection_feed(activs, confs, picked, proj_net, first_level=OFFSET)
    logits = torch.cat([cl.movedim(1, 3).reshape(B, -1).gather(1, s.long()) for cl, s in zip(confs, picked)], dim=1).reshape(-1)
    assert torch.equal(logits.detach(), conf.reshape(-1))
    proj_embds = proj_net(feed)
    proj_embds = proj_embds.reshape(-1, proj_embds.shape[-1])
    dm, da = proj_net.dot_mult, proj_net.dot_add
    sel = episode.cluster(proj_embds, conf.reshape(-1), B, dm, da)
    assert int(sel['n_valid']) > 0
    supp = episode.support_loss(proj_embds.detach() if stop_grad else proj_embds, logits, logits, sel, dm, da)
    loss = outer(params, head_gpu, supp['loss'], [t.to(DEV) for t in qry_x])
    loss.backward()
    proj_params = [m.weight for m in proj_net.projection if isinstance(m, torch.nn.Linear)]
    # ---- CPU replica
    head_cpu = lambda ps, x: tip._oracle_head(c, mh_names, ps, x)
    outs_r, activs_r = head_cpu(ref_params, [t.clone() for t in c['x']])
    masks = [torch.zeros(B, o.shape[1] * o.shape[2] * o.shape[3], dtype=torch.bool).scatter_(1, s.cpu().long(), True)
             for o, s in zip(outs_r, picked)]
    enc = [t.cpu() for t in (proj_net.anch_enc, proj_net.lev_enc, proj_net.cell_enc)]
    feed_r, conf_r, _ = ref.episode_feed(activs_r, outs_r, *enc, first_level=OFFSET, masks=masks)
    embds_r = om.projection_forward(proj_ref, feed_r.detach().reshape(-1, feed_r.shape[-1]))
    sel_cpu = {k: sel[k].cpu() for k in ('proto0', 'valid', 'proto', 'nearest')}
    logits_r = conf_r.reshape(-1)
    supp_r, target_r = sref.loss_literal(embds_r.detach() if stop_grad else embds_r, logits_r, logits_r, sel_cpu, dots_ref[0], dots_ref[1], B)
    loss_r = outer(ref_params, head_cpu, supp_r, qry_x)
    print('support loss %.6g, replica %.6g; query loss %.6g, replica %.6g' % (float(supp['loss']), float(supp_r), float(loss), float(loss_r)))
    assert abs(float(supp['loss'].detach()) - float(supp_r.detach())) <= 1e-3 * abs(float(supp_r.detach()))
    assert abs(float(loss.detach()) - float(loss_r.detach())) <= 1e-3 * max(1e-3, abs(float(loss_r.detach())))
    gr = torch.autograd.grad(loss_r, proj_ref + ref_params, allow_unused=True)
    if stop_grad:
        assert all(p.grad is None for p in proj_params) and all(g is None for g in gr[:len(proj_params)])
    else:
        for p in proj_params:
            assert p.grad is not None and float(p.grad.abs().max()) > 0
        tip._compare([p.grad for p in proj_params], gr[:len(proj_params)], 1e-3, 'proj_net')
    used = [(p.grad, r_) for p, r_ in zip(mh.parameters(), gr[len(proj_params):]) if r_ is not None]
    tip._compare([g for g, _ in used], [r_ for _, r_ in used], 1e-3, 'class_net')
