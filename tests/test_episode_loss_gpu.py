"""episode.projection_losses (csrc/episode_loss.hip) against the float64 lean form of tests/_episode_loss_ref.py, which
tests/test_episode_loss_host.py shows equal to the literal n x n form of infer.py:448-494.

Inputs.  Rows from _episode_ref.clustered_rows, confs ~ N(0, 1) with dot_mult 1.5, dot_add 0.25, labels drawn from
{-2, -1, -1, 0, c, c, c, 9} with c = cls_id = 5.  The decisions are the float64 cluster_lean ones, uploaded, so nothing here
depends on float32 argmax ties; the seeds are those for which decision_gaps passes test_episode_gpu.py's thresholds and at
least 3 prototypes are valid.

Bounds.  Values: 2e-5 of max|ref| (test_episode_gpu._close's bound; the float32 literal form on the CPU measured 7.4e-7).
Gradients: 1e-4 of the largest entry of that gradient in the float64 reference (the float32 literal form measured 7.5e-7; the
room is for another summation order over n rows).  Hinge kinks: K = the rows whose float64 hinge argument is within 1e-5 of 0 (in
'no_conf' every prototype row with a positive target, its sim being exactly 1).  float32 may land on either side there, so with
G0 the reference gradient with those rows switched off and D_r the change row r makes when switched on, the device gradient must
lie entrywise in [G0 + sum_r min(0, D_r) - tol, G0 + sum_r max(0, D_r) + tol]; |K| <= m + 4 is asserted on the reference alone."""
import functools
import itertools
import types

import pytest
import torch

import _episode_loss_ref as lref
import _episode_ref as ref
from _episode_cases import DEV, NUM_IMAGES, OFFSET, _device_sel, _levels, _meta_head, _same

pytestmark = pytest.mark.gpu

CLS = lref.CLS_ID
CONFIGS = [('max', 'separate'), ('max', 'same'), ('max', 'no_conf'), ('avg', 'separate')]
SIZES = [(25, 252, 256, 2), (7, 100, 64, 3), (64, 5, 256, 4), (5, 37, 100, 6)]        # num, rows, d, clustered_rows seed
PROJ_SIZE = (25, 1692, 256, 5)
WEIGHTS = (0.7, 0.7, 0.01)                                                              # upstream of clust, embds, obj


@functools.lru_cache(maxsize=None)
def _inputs(num, rows, d, seed, sim_target, saturated=False):
    """-> x [n, d], confs [n] (float32, CPU), dot_mult, dot_add, decisions of the float64 lean form"""
    x, sat_confs = ref.clustered_rows(seed, num, rows, d)
    if saturated:
        confs, dm, da = sat_confs, 3., 3.                                               # the cluster tests' recipe: |l| beyond 18
    else:
        confs, dm, da = torch.randn(num * rows, generator=torch.Generator().manual_seed(seed)), 1.5, 0.25
    sel, lean = lref.decisions(x.double(), confs.double(), dm, da, num, sim_target)
    rel, margin, _ = ref.decision_gaps(lean)
    assert rel >= 1e-5 and margin >= 1e-4 and int(sel['valid'].sum()) >= 3, (rel, margin, int(sel['valid'].sum()))
    return x, confs, dm, da, sel


@functools.lru_cache(maxsize=None)
def _labels(seed, n, first_is_task, pool=lref.LABEL_POOL):
    return lref.draw_labels(seed, n, first_is_task, pool)


def _gpu(x, confs, labs, sel, dm, da, sim_target, loss_mode, margin, cls=CLS, grad=True, weights=WEIGHTS):
    from ood_object_detection_amd import episode
    leaves = [x.to(DEV, copy=True).requires_grad_(grad), confs.to(DEV, copy=True).requires_grad_(grad),
              torch.tensor(dm, device=DEV, requires_grad=grad), torch.tensor(da, device=DEV, requires_grad=grad)]
    out = episode.projection_losses(leaves[0], leaves[1], labs.to(DEV), cls, _device_sel(sel), leaves[2], leaves[3], sim_target, loss_mode, margin)
    grads = None
    if grad:
        total = weights[0] * out['clust_loss'] + weights[1] * out['embds_loss'] + weights[2] * out['obj_loss']
        grads = torch.autograd.grad(total, leaves)
    return out, grads


def _ref64(x, confs, labs, sel, dm, da, sim_target, loss_mode, margin, a=None, weights=WEIGHTS, grad=True):
    leaves = [x.double().clone().requires_grad_(grad), confs.double().clone().requires_grad_(grad),
              torch.tensor(dm, dtype=torch.float64, requires_grad=grad), torch.tensor(da, dtype=torch.float64, requires_grad=grad)]
    out = lref.losses_lean(leaves[0], leaves[1], labs, CLS, sel, leaves[2], leaves[3], sim_target, loss_mode, margin, a=a)
    grads = None
    if grad:
        total = weights[0] * out['clust_loss'] + weights[1] * out['embds_loss'] + weights[2] * out['obj_loss']
        grads = torch.autograd.grad(total, leaves)
    return out, grads


def _close(got, want, what, scale=None):
    want = torch.as_tensor(want).float()
    scale = float(want.abs().max()) if scale is None else scale
    err = float((torch.as_tensor(got).detach().cpu().float() - want).abs().max())
    print('%s: max err %.3e, max|ref| %.3e' % (what, err, scale))
    assert err <= 2e-5 * scale, (what, err, scale)


def _check_values(out, want, what):
    for k in ('clust_loss', 'embds_loss', 'obj_loss', 'inner_target'):
        _close(out[k], want[k].detach(), '%s %s' % (what, k))
    got_stats = torch.stack([out['stats'][k] for k in lref.STAT_NAMES]).cpu()
    want_stats = torch.stack([want['stats'][k] for k in lref.STAT_NAMES]).float()
    nan = torch.isnan(want_stats)
    assert torch.equal(torch.isnan(got_stats), nan), what
    _close(got_stats[~nan], want_stats[~nan], what + ' stats')
    assert out['counts'].dtype == torch.int32 and out['counts'].cpu().tolist() == want['counts'], what
    assert not out['inner_target'].requires_grad


def _kink_rows(want, m):
    K = torch.nonzero(want['embds_arg'].abs() <= 1e-5).reshape(-1)
    assert K.numel() <= m + 4, K.numel()
    if want['clust_arg'] is not None:
        assert float(want['clust_arg'].abs().min()) > 1e-5          # the m-term hinge has no kink in these cases
    return K


def _check_gradients(got, case, labs, sel, config, margin, bound, what, want=None, m=None):
    """the interval comparison of the module docstring"""
    x, confs, dm, da = case
    sim_target, loss_mode = config
    if want is None:
        want, _ = _ref64(x, confs, labs, sel, dm, da, sim_target, loss_mode, margin, grad=False)
    K = _kink_rows(want, sel['proto'].numel() if m is None else m)
    a0 = (want['embds_arg'] >= 0).double()
    a0[K] = 0.
    _, g_full = _ref64(x, confs, labs, sel, dm, da, sim_target, loss_mode, margin)
    _, g0 = _ref64(x, confs, labs, sel, dm, da, sim_target, loss_mode, margin, a=a0)
    lo, hi = [g.clone() for g in g0], [g.clone() for g in g0]
    for r in K.tolist():
        a = a0.clone()
        a[r] = 1.
        _, gr = _ref64(x, confs, labs, sel, dm, da, sim_target, loss_mode, margin, a=a)
        for i in range(len(g0)):
            dr = gr[i] - g0[i]
            lo[i] += dr.clamp(max=0)
            hi[i] += dr.clamp(min=0)
    for i, name in enumerate(('d embds', 'd confs', 'd dot_mult', 'd dot_add')):
        g = got[i].detach().cpu().double()
        assert bool(torch.isfinite(g).all()), (what, name)
        scale = float(g_full[i].abs().max())
        tol = bound * scale
        err = float(torch.maximum(lo[i] - g, g - hi[i]).clamp(min=0).max())
        print('%s %s: |K| %d, outside the interval by %.3e, largest entry %.3e' % (what, name, K.numel(), err, scale))
        assert scale > 0 and err <= tol, (what, name, err, scale)


def _each(num, rows, d, seed, config):
    sim_target, loss_mode = config
    x, confs, dm, da, sel = _inputs(num, rows, d, seed, sim_target)
    for margin, first in itertools.product((0., 0.1), (True, False)):
        labs = _labels(seed, num * rows, first)
        yield (x, confs, dm, da), sel, labs, margin, first


# ---- 1. values ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('config', CONFIGS, ids=lambda c: '-'.join(c))
@pytest.mark.parametrize('num,rows,d,seed', SIZES)
def test_values(num, rows, d, seed, config):
    for case, sel, labs, margin, first in _each(num, rows, d, seed, config):
        want, _ = _ref64(*case[:2], labs, sel, *case[2:], *config, margin, grad=False)
        out, _ = _gpu(*case[:2], labs, sel, *case[2:], *config, margin, grad=False)
        assert min(want['counts']) > 0
        assert (want['positives'] > 0) == (first or config[0] == 'avg')
        _check_values(out, want, '%s margin %g first %s' % (config, margin, first))


def test_values_without_other_objects():
    num, rows, d, seed = SIZES[1]
    x, confs, dm, da, sel = _inputs(num, rows, d, seed, 'max')
    labs = _labels(seed, num * rows, True, pool=(-2, -1, -1, CLS, CLS, CLS))
    want, _ = _ref64(x, confs, labs, sel, dm, da, 'max', 'separate', 0., grad=False)
    out, _ = _gpu(x, confs, labs, sel, dm, da, 'max', 'separate', 0., grad=False)
    assert want['counts'][1] == 0 and int(out['counts'][1]) == 0
    assert bool(torch.isnan(out['stats']['other_obj_mean'])) and bool(torch.isnan(out['stats']['other_obj_max']))
    _check_values(out, want, 'no other object')


# ---- 2. gradients ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('config', CONFIGS, ids=lambda c: '-'.join(c))
@pytest.mark.parametrize('num,rows,d,seed', SIZES)
def test_gradients(num, rows, d, seed, config):
    for case, sel, labs, margin, first in _each(num, rows, d, seed, config):
        _, grads = _gpu(*case[:2], labs, sel, *case[2:], *config, margin)
        _check_gradients(grads, case, labs, sel, config, margin, 1e-4, '%s margin %g first %s' % (config, margin, first))


# ---- 3. saturated confidences ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('num,rows,d,seed', SIZES[:2])
def test_saturated_confidences(num, rows, d, seed):
    x, confs, dm, da, sel = _inputs(num, rows, d, seed, 'max', saturated=True)
    labs = _labels(seed, num * rows, True)
    assert float((dm * (confs + da)).abs().max()) > 15              # sigmoid within float32 resolution of 0 / 1 (18.6 and 23.9 here)
    want, _ = _ref64(x, confs, labs, sel, dm, da, 'max', 'separate', 0., grad=False)
    out, grads = _gpu(x, confs, labs, sel, dm, da, 'max', 'separate', 0.)
    _check_values(out, want, 'saturated')
    assert all(bool(torch.isfinite(g).all()) for g in grads)
    only_obj = (0., 0., 1.)
    _, g_obj = _gpu(x, confs, labs, sel, dm, da, 'max', 'separate', 0., weights=only_obj)
    _, want_obj = _ref64(x, confs, labs, sel, dm, da, 'max', 'separate', 0., weights=only_obj)
    assert float(g_obj[0].abs().max()) == 0. and float(want_obj[0].abs().max()) == 0.            # obj_loss does not see the embeddings
    for i, name in ((1, 'd confs'), (2, 'd dot_mult'), (3, 'd dot_add')):
        scale = float(want_obj[i].abs().max())
        err = float((g_obj[i].cpu().double() - want_obj[i]).abs().max())
        print('obj_loss alone %s: max err %.3e, largest entry %.3e' % (name, err, scale))
        assert err <= 1e-4 * scale


# ---- 4. projection-phase size ------------------------------------------------------------------------------------------------------

def test_projection_phase_size_without_an_n_by_n_buffer():
    from ood_object_detection_amd import episode
    num, rows, d, seed = PROJ_SIZE
    x, confs, dm, da, sel = _inputs(num, rows, d, seed, 'max')
    n = num * rows
    labs = _labels(seed, n, True)
    xg, cg, lg, sg = x.to(DEV).requires_grad_(), confs.to(DEV).requires_grad_(), labs.to(DEV), _device_sel(sel)
    dmg, dag = torch.tensor(dm, device=DEV, requires_grad=True), torch.tensor(da, device=DEV, requires_grad=True)
    small = dict(proto0=torch.arange(num, device=DEV), proto=torch.arange(num, device=DEV), valid=sg['valid'], nearest=sg['nearest'][:num * 4])
    w = episode.projection_losses(xg[:num * 4], cg[:num * 4], lg[:num * 4], CLS, small, dmg, dag)    # library loaded, allocator warm
    torch.autograd.grad(w['embds_loss'] + w['obj_loss'], [xg, cg, dmg, dag])
    del w
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    out = episode.projection_losses(xg, cg, lg, CLS, sg, dmg, dag, 'max', 'separate', 0.)
    total = WEIGHTS[0] * out['clust_loss'] + WEIGHTS[1] * out['embds_loss'] + WEIGHTS[2] * out['obj_loss']
    grads = torch.autograd.grad(total, [xg, cg, dmg, dag])
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    input_bytes = xg.numel() * 4 + cg.numel() * 4 + lg.numel() * 8
    print('peak memory grew by %d bytes across forward + backward, inputs are %d bytes (%.2f x)' % (grown, input_bytes, grown / input_bytes))
    assert grown < 4 * input_bytes                                  # one n x n float32 matrix would be 165 x the inputs
    want, _ = _ref64(x, confs, labs, sel, dm, da, 'max', 'separate', 0., grad=False)
    _check_values(out, want, 'projection-phase size')
    _check_gradients(grads, (x, confs, dm, da), labs, sel, ('max', 'separate'), 0., 1e-4, 'projection-phase size', want=want)


# ---- 5. determinism and capture ----------------------------------------------------------------------------------------------------

def _flat(out, grads):
    return [out['clust_loss'], out['embds_loss'], out['obj_loss'], out['inner_target'], out['counts']] + \
        [out['stats'][k] for k in lref.STAT_NAMES] + list(grads)


@pytest.mark.parametrize('config', [('max', 'same'), ('avg', 'separate')], ids=lambda c: '-'.join(c))
def test_two_calls_give_the_same_bits_and_device_scalars_too(config):
    num, rows, d, seed = SIZES[0]
    x, confs, dm, da, sel = _inputs(num, rows, d, seed, config[0])
    labs = _labels(seed, num * rows, True)
    first = _flat(*_gpu(x, confs, labs, sel, dm, da, *config, 0.1))
    again = _flat(*_gpu(x, confs, labs, sel, dm, da, *config, 0.1))
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    # numbers instead of device tensors for dot_mult / dot_add, a device tensor for cls_id: the same bits
    from ood_object_detection_amd import episode
    xg, cg = x.to(DEV).requires_grad_(), confs.to(DEV).requires_grad_()
    out = episode.projection_losses(xg, cg, labs.to(DEV), torch.tensor(CLS, device=DEV), _device_sel(sel), dm, da, *config, 0.1)
    total = WEIGHTS[0] * out['clust_loss'] + WEIGHTS[1] * out['embds_loss'] + WEIGHTS[2] * out['obj_loss']
    grads = torch.autograd.grad(total, [xg, cg])
    assert all(torch.equal(a, b) for a, b in zip(first[:-2], _flat(out, grads)))


def test_chain_with_losses_and_backward_in_one_graph_replays_bit_for_bit():
    from ood_object_detection_amd import episode
    from ood_object_detection_amd.effdet.efficientdet import ProjectionNet
    B, Fc, sides = 5, 64, [16, 8, 4]
    torch.manual_seed(3)
    proj_net = ProjectionNet(types.SimpleNamespace(fpn_channels=Fc), 128).to(DEV)
    rows = sum(episode.kept_per_level(s, s) for s in sides)

    def chain(activs, confs, labs):
        with torch.no_grad():
            sel = episode.select_anchors(confs)
            feed, conf = episode.projection_feed(activs, confs, sel, proj_net, first_level=OFFSET)
            embds = proj_net(feed).reshape(-1, 64)
            out = episode.cluster(embds, conf.reshape(-1), B, proj_net.dot_mult, proj_net.dot_add)
        embds = embds.detach().requires_grad_()
        logits = conf.reshape(-1).detach().requires_grad_()
        dm, da = proj_net.dot_mult.detach().requires_grad_(), proj_net.dot_add.detach().requires_grad_()
        loss = episode.projection_losses(embds, logits, labs, CLS, out, dm, da, 'max', 'separate', 0.)
        total = 0.03 * (30. * (loss['embds_loss'] + loss['clust_loss']) + 1e-4 * loss['obj_loss'])
        return _flat(loss, torch.autograd.grad(total, [embds, logits, dm, da]))

    a1, c1 = _levels(31, B, Fc, sides)
    a2, c2 = _levels(32, B, Fc, sides)
    l1, l2 = _labels(31, B * rows, True).to(DEV), _labels(32, B * rows, True).to(DEV)
    static_a = [t.clone(memory_format=torch.preserve_format) for t in a1]
    static_c = [t.clone(memory_format=torch.preserve_format) for t in c1]
    static_l = l1.clone()
    eager1 = [t.clone() for t in chain(a1, c1, l1)]
    eager2 = [t.clone() for t in chain(a2, c2, l2)]
    assert bool(torch.isfinite(eager1[1])) and float(eager1[-4].abs().max()) > 0 and not torch.equal(eager1[-4], eager2[-4])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain(static_a, static_c, static_l)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = chain(static_a, static_c, static_l)
    for (na, nc, nl), eager in (((a2, c2, l2), eager2), ((a1, c1, l1), eager1)):
        for s, t in zip(static_a, na):
            s.copy_(t)
        for s, t in zip(static_c, nc):
            s.copy_(t)
        static_l.copy_(nl)
        graph.replay()
        torch.cuda.synchronize()
        assert _same(captured, eager)


# ---- 6. empty valid set ------------------------------------------------------------------------------------------------------------

def test_empty_valid_set_gives_nan_clust_loss_and_a_finite_obj_loss():
    num, rows, d, seed = SIZES[1]
    x, confs, dm, da, sel = _inputs(num, rows, d, seed, 'max')
    labs = _labels(seed, num * rows, True)
    empty = dict(sel, valid=torch.zeros_like(sel['valid']))
    want, _ = _ref64(x, confs, labs, sel, dm, da, 'max', 'separate', 0., grad=False)
    out, _ = _gpu(x, confs, labs, empty, dm, da, 'max', 'separate', 0., grad=False)
    assert bool(torch.isnan(out['clust_loss'])) and bool(torch.isnan(out['inner_target']).all())
    assert bool(torch.isfinite(out['obj_loss']))
    _close(out['obj_loss'], want['obj_loss'].detach(), 'obj_loss with an empty valid set')
    _close(out['embds_loss'], want['embds_loss'].detach(), "'separate' embds_loss does not read target_clust")
    assert all(bool(torch.isnan(out['stats'][k])) for k in lref.STAT_NAMES) and out['counts'].cpu().tolist() == want['counts']


# ---- 7. end to end -------------------------------------------------------------------------------------------------------------------

def _final_loss(o):
    return 0.03 * (30. * (o['embds_loss'] + o['clust_loss']) + 1e-4 * o['obj_loss'])       # infer.py:787-789, default coefficients


def test_end_to_end_projection_phase_step(golden):
    """select_anchors, projection_feed, proj_net, cluster, projection_losses, backward - against a CPU replica through the oracle that
    is given the GPU's decisions.  The feed is a copy without history (FLAGS.proj_stop_grad); the MetaHead gets its gradient
    through the confidences, gathered with the selection."""
    from oracle import model as om
    from ood_object_detection_amd import episode
    c, mh, proj_net, xs = _meta_head(golden, 21, with_case=True)
    confs, activs = mh([t.to(DEV) for t in xs], ret_activs=True, level_offset=OFFSET)
    sel = episode.select_anchors(confs)
    feed, conf = episode.projection_feed(activs, confs, sel, proj_net, first_level=OFFSET)
    logits = torch.cat([cl.movedim(1, 3).reshape(NUM_IMAGES, -1).gather(1, s.long()) for cl, s in zip(confs, sel)], dim=1)
    assert torch.equal(logits.detach(), conf) and feed.shape[:2] == (NUM_IMAGES, 252)
    proj_embds = proj_net(feed).reshape(-1, 256)
    dm, da = proj_net.dot_mult, proj_net.dot_add
    out = episode.cluster(proj_embds, conf.reshape(-1), NUM_IMAGES, dm, da)
    n = NUM_IMAGES * 252
    labs = _labels(21, n, True)
    loss = episode.projection_losses(proj_embds, logits.reshape(-1), labs.to(DEV), CLS, out, dm, da, 'max', 'separate', 0.)
    _final_loss(loss).backward()
    weights = [m.weight for m in proj_net.projection if isinstance(m, torch.nn.Linear)]
    got = [w.grad for w in weights] + [dm.grad, da.grad, mh.predict_pw.grad, mh.conv_pw0.grad]
    # ---- CPU replica
    names = [k for k, _ in mh.named_parameters()]
    ref_params = [p.detach().cpu().clone().requires_grad_() for p in mh.parameters()]
    f = dict(zip(names, ref_params))
    R, L = c['R'], c['L']
    outs_r, activs_r = om.meta_head_forward([f['conv_dw%d' % r] for r in range(R)], [f['conv_pw%d' % r] for r in range(R)],
                                            [f['conv_pb%d' % r] for r in range(R)],
                                            [f['bn_w%d%d' % (r, lev)] for lev in range(L) for r in range(R)],
                                            [f['bn_b%d%d' % (r, lev)] for lev in range(L) for r in range(R)],
                                            [f['predict_dw'], f['predict_pw'], f['predict_pb']], [t.clone() for t in xs], level_offset=OFFSET)
    masks = [torch.zeros(NUM_IMAGES, o.shape[1] * o.shape[2] * o.shape[3], dtype=torch.bool).scatter_(1, s.cpu().long(), True)
             for o, s in zip(outs_r, sel)]
    enc = [t.cpu() for t in (proj_net.anch_enc, proj_net.lev_enc, proj_net.cell_enc)]
    feed_r, conf_r, _ = ref.episode_feed(activs_r, outs_r, *enc, first_level=OFFSET, masks=masks)
    w_ref = [w.detach().cpu().clone().requires_grad_() for w in weights]
    dots_ref = [dm.detach().cpu().clone().requires_grad_(), da.detach().cpu().clone().requires_grad_()]
    embds_r = om.projection_forward(w_ref, feed_r.detach().reshape(-1, feed_r.shape[-1]))
    sel_gpu = {k: out[k].cpu() for k in ('proto0', 'valid', 'proto', 'nearest')}
    wrt = w_ref + dots_ref + [f['predict_pw'], f['conv_pw0']]

    def replica(a=None):
        o = lref.losses_lean(embds_r, conf_r.reshape(-1), labs, CLS, sel_gpu, dots_ref[0], dots_ref[1], 'max', 'separate', 0., a=a)
        return o, torch.autograd.grad(_final_loss(o), wrt, retain_graph=True)

    want, g_full = replica()
    for k in ('clust_loss', 'embds_loss', 'obj_loss'):
        err = abs(float(loss[k].detach()) - float(want[k].detach()))
        print('%s: %.6g, replica %.6g' % (k, float(loss[k].detach()), float(want[k].detach())))
        assert err <= 1e-3 * abs(float(want[k].detach())), k
    K = _kink_rows(want, NUM_IMAGES)
    a0 = (want['embds_arg'] >= 0).float()
    a0[K] = 0.
    _, g0 = replica(a0)
    lo, hi = [g.clone() for g in g0], [g.clone() for g in g0]
    for r in K.tolist():
        a = a0.clone()
        a[r] = 1.
        _, gr = replica(a)
        for i in range(len(g0)):
            lo[i] += (gr[i] - g0[i]).clamp(max=0)
            hi[i] += (gr[i] - g0[i]).clamp(min=0)
    for i, name in enumerate(['proj_net weight %d' % j for j in range(len(weights))] + ['dot_mult', 'dot_add', 'predict_pw', 'conv_pw0']):
        g = got[i].detach().cpu()
        scale = float(g_full[i].abs().max())
        err = float(torch.maximum(lo[i] - g, g - hi[i]).clamp(min=0).max())
        print('%s: |K| %d, outside the interval by %.3e, largest entry %.3e' % (name, K.numel(), err, scale))
        assert bool(torch.isfinite(g).all()) and scale > 0 and err <= 1e-3 * scale, (name, err, scale)
