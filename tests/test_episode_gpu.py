"""The episode stage on the device (ood_object_detection_amd/episode.py, csrc/episode.hip) against the literal restatements of
infer.py:362-447 / :566-654 in tests/_episode_ref.py.

Bounds.  Copies (selection, feed) are exact.  Continuous quantities of the cluster stage are within 2e-5 of max|ref| (DESIGN §2's
bound for float32 kernels).  Discrete decisions are exact wherever the float64 reference itself decides by a clear margin: every
per-image top-2 gap >= 1e-5 of max|score| and every validity margin >= 1e-4 (asserted on the reference alone, the seeds are
chosen to meet it); the per-row nearest prototype is exact on the rows whose float64 top-2 gap exceeds 1e-4, and at most 2 % of
the rows may fall below that."""
import types

import pytest
import torch
import torch.nn.functional as F

import _episode_ref as ref
from _episode_cases import A, DEV, NUM_IMAGES, OFFSET, _head_like, _levels, _meta_head, _same

pytestmark = pytest.mark.gpu


def _proj_net(fpn_channels, width=64, seed=0):
    from ood_object_detection_amd.effdet.efficientdet import ProjectionNet
    torch.manual_seed(seed)
    return ProjectionNet(types.SimpleNamespace(fpn_channels=fpn_channels), width).to(DEV)


# ---- 1. selection -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('B', [25, 3])
@pytest.mark.parametrize('side', [8, 16, 32, 64, 5])
def test_selection_matches_the_quantile_mask(side, B):
    from ood_object_detection_amd import episode
    N = A * side * side
    res_conf = ref.tie_free_confs(100 * side + B, B, N)
    assert ref.tie_free(res_conf)
    mask = ref.quantile_mask(res_conf, side)
    want = ref.mask_indices(mask)
    assert want.shape == (B, episode.kept_per_level(side, side))
    conf = _head_like(res_conf, side)
    got = episode.select_anchors([conf])[0]
    assert got.dtype == torch.int32 and got.shape == want.shape
    assert torch.equal(got.cpu().long(), want)
    flat = conf.movedim(1, 3).reshape(B, -1)
    assert torch.equal(torch.gather(flat, 1, got.long()).cpu(), res_conf[mask].reshape(B, -1))
    # an NCHW-contiguous tensor (not the head's memory order) gives the same selection
    assert torch.equal(episode.select_anchors([conf.contiguous()])[0], got)


def test_selection_of_several_levels_and_small_maps_keep_all():
    from ood_object_detection_amd import episode
    B, sides = 4, [16, 8, 4, 2, 1]
    res = [ref.tie_free_confs(7 + s, B, A * s * s) for s in sides]
    got = episode.select_anchors([_head_like(r, s) for r, s in zip(res, sides)])
    for g, r, s in zip(got, res, sides):
        assert torch.equal(g.cpu().long(), ref.mask_indices(ref.quantile_mask(r, s)))
        if s <= 4:
            assert torch.equal(g.cpu().long(), torch.arange(A * s * s).repeat(B, 1))


def test_selection_ties_go_to_the_lower_index():
    from ood_object_detection_amd import episode
    B, side = 3, 8
    N, keep = A * side * side, episode.kept_per_level(side, side)
    gen = torch.Generator().manual_seed(5)
    res_conf = torch.zeros(B, N)
    for b, ones in enumerate((50, 0, keep)):                     # 50 clear winners + 22 of the tied; all tied; no tied one kept
        res_conf[b, torch.randperm(N, generator=gen)[:ones]] = 1.0
    res_conf[1] = -0.0                                            # -0 == +0
    res_conf[1, 7] = 0.0
    order = torch.sort(res_conf, dim=1, descending=True, stable=True)[1][:, :keep]
    want = torch.sort(order, dim=1)[0]
    got = episode.select_anchors([_head_like(res_conf, side)])[0]
    assert torch.equal(got.cpu().long(), want)
    assert torch.equal(want[1], torch.arange(keep))


# ---- 2. feed ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('first_level,sides', [(0, [16, 8, 4, 2]), (2, [8, 4, 2])])
@pytest.mark.parametrize('Fc', [64, 88, 160, 66])            # 66: no 16-byte pieces, the kernel's scalar copy
def test_feed_is_the_literal_expression_bit_for_bit(Fc, first_level, sides):
    from ood_object_detection_amd import episode
    B = 3
    proj_net = _proj_net(Fc)
    activs, confs = _levels(11 + Fc, B, Fc, sides)
    want_feed, want_conf, masks = ref.episode_feed(activs, confs, proj_net.anch_enc, proj_net.lev_enc, proj_net.cell_enc, first_level)
    sel = episode.select_anchors(confs)
    for s, m in zip(sel, masks):
        assert torch.equal(s.long(), ref.mask_indices(m))
    feed, conf = episode.projection_feed(activs, confs, sel, proj_net, first_level=first_level)
    K, Kp = Fc + 42, (Fc + 42 + 7) // 8 * 8
    assert feed.shape == want_feed.shape == (B, sum(s.shape[1] for s in sel), K) and feed.stride() == (feed.shape[1] * Kp, Kp, 1)
    assert torch.equal(feed, want_feed) and torch.equal(conf, want_conf)
    full = torch.as_strided(feed, (B, feed.shape[1], Kp), feed.stride())
    assert bool((full[..., K:] == 0).all())
    with torch.no_grad():
        pitched = proj_net(feed)
        packed = proj_net(feed.contiguous())
    assert pitched.shape == (B, feed.shape[1], 32) and torch.equal(pitched, packed)


# ---- 3. / 4. cluster ----------------------------------------------------------------------------------------------------------

def _close(got, want, what):
    want = want.float()
    scale = float(want.abs().max())
    err = float((got.cpu() - want).abs().max())
    print('%s: max err %.3e, max|ref| %.3e' % (what, err, scale))
    assert err <= 2e-5 * scale, (what, err, scale)


def _check_cluster(out, lit, lean64, sim_target, novelty, max_skipped=0.02):
    """lit: the float32 literal form (None where it cannot run: the float64 lean form stands in); lean64: the float64 lean form,
    which supplies the decisions and their margins"""
    rel, margin, row_gap = ref.decision_gaps(lean64)
    print('reference alone: top-2 gap %.2e of max|score|, validity margin %.2e' % (rel, margin))
    assert rel >= 1e-5 and margin >= 1e-4                        # the float64 reference decides clearly
    assert 0 < int(lean64['valid'].sum()) == int(out['n_valid'].cpu())
    for k in ('proto0', 'valid', 'proto'):
        assert torch.equal(out[k].cpu(), lean64[k]), k
        if lit is not None:
            assert torch.equal(lit[k], lean64[k]), k
    src = lit if lit is not None else lean64
    for k in ('soft_thresh', 'avg_init0', 'avg_init', 'target_clust', 'sim'):
        _close(out[k], src[k], k)
    # target carries target_clust[nearest]: compared where both sides name the same prototype (every clear row, see below)
    agree = out['nearest'].cpu() == src['nearest'] if sim_target == 'max' else torch.ones_like(src['target'], dtype=torch.bool)
    _close(torch.where(agree, out['target'].cpu(), torch.zeros(())), torch.where(agree, src['target'].float(), torch.zeros(())), 'target')
    if sim_target == 'max':
        assert bool(agree[row_gap > 1e-4].all())
        clear = row_gap > 1e-4
        skipped = 1.0 - float(clear.double().mean())
        print('rows below the 1e-4 gap: %.2f %%' % (100 * skipped))
        assert max_skipped is None or skipped <= max_skipped
        near = out['nearest'].cpu()
        assert torch.equal(near[clear], lean64['nearest'][clear])
        # every row, clear or not: the prototype picked is within float32 resolution of the reference's best
        picked = torch.gather(lean64['cols'], 1, near.reshape(-1, 1)).reshape(-1)
        assert float((lean64['cols'].max(1)[0] - picked).max()) <= 2e-5
    _close(novelty['sim'], src['sim'], 'novelty_score sim')
    print('novelty_score sim bit-equal:', torch.equal(novelty['sim'], out['sim']))
    assert float((novelty['sim'] - out['sim']).abs().max()) <= 1e-6


CLUSTER_CASES = [(25, 252, 256, 2), (7, 100, 64, 3)]            # num_images, rows, d, seed (see the module docstring)


@pytest.mark.parametrize('sim_target', ['max', 'avg'])
@pytest.mark.parametrize('valid_threshold', [None, 0.3])
@pytest.mark.parametrize('num,rows,d,seed', CLUSTER_CASES)
def test_cluster_against_the_literal_form(num, rows, d, seed, valid_threshold, sim_target):
    from ood_object_detection_amd import episode, ood
    x, confs = ref.clustered_rows(seed, num, rows, d)
    lit = ref.cluster_literal(x, confs, 3., 3., num, valid_threshold, sim_target)
    lean64 = ref.cluster_lean(x.double(), confs.double(), 3., 3., num, valid_threshold, sim_target)
    xg, cg = x.to(DEV), confs.to(DEV)
    out = episode.cluster(xg, cg, num, 3., 3., valid_threshold, sim_target)
    nov = ood.novelty_score(xg, cg, out['proto'], 3., 3., sim_target)
    _check_cluster(out, lit, lean64, sim_target, nov)
    # dot_mult / dot_add as device tensors (proj_net's parameters) give the same bits
    out_t = episode.cluster(xg, cg, num, torch.tensor(3., device=DEV), torch.tensor(3., device=DEV), valid_threshold, sim_target)
    for k in out:
        assert torch.equal(out[k], out_t[k]), k


def test_cluster_empty_valid_set_gives_nan_and_says_so():
    from ood_object_detection_amd import episode
    x, confs = ref.clustered_rows(3, 7, 100, 64)
    out = episode.cluster(x.to(DEV), confs.to(DEV), 7, 3., 3., valid_threshold=2.0)
    assert int(out['n_valid'].cpu()) == 0 and not bool(out['valid'].any())
    assert bool(torch.isnan(out['target_clust']).all()) and bool(torch.isnan(out['target']).all())
    assert bool(torch.isfinite(out['sim']).all()) and bool(torch.isfinite(out['avg_init']).all())
    assert torch.equal(out['proto'].cpu(), torch.arange(0, 700, 100))


def test_cluster_at_the_projection_phase_size_without_an_n_by_n_buffer():
    from ood_object_detection_amd import episode, ood
    num, rows, d, seed = 25, 1692, 256, 5
    x, confs = ref.clustered_rows(seed, num, rows, d)
    lean64 = ref.cluster_lean(x.double(), confs.double(), 3., 3., num, None, 'max')
    xg, cg = x.to(DEV), confs.to(DEV)
    episode.cluster(xg[:num * 4], cg[:num * 4], num, 3., 3.)                  # library loaded, allocator warm
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    out = episode.cluster(xg, cg, num, 3., 3.)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    input_bytes = xg.numel() * 4 + cg.numel() * 4
    print('peak memory grew by %d bytes across the call, inputs are %d bytes' % (grown, input_bytes))
    assert grown < 4 * input_bytes                                             # one n x n float32 matrix would be 165 x the inputs
    nov = ood.novelty_score(xg, cg, out['proto'], 3., 3., 'max')
    _check_cluster(out, None, lean64, 'max', nov)


# ---- 5. end to end ------------------------------------------------------------------------------------------------------------

def _e2e_loss(target, conf_logits):
    return F.binary_cross_entropy_with_logits(conf_logits, target)              # infer.py:656


def test_end_to_end_episode_stage(golden):
    from oracle import model as om
    from ood_object_detection_amd import episode, ood
    mh, proj_net, xs = _meta_head(golden, 21)
    with torch.no_grad():
        confs, activs = mh([t.to(DEV) for t in xs], ret_activs=True, level_offset=OFFSET)
    sel = episode.select_anchors(confs)
    feed, conf = episode.projection_feed(activs, confs, sel, proj_net, first_level=OFFSET)
    assert feed.shape[:2] == (NUM_IMAGES, 252)
    proj_embds = proj_net(feed).reshape(-1, 256)                                # with autograd history (float32 training kernels)
    dm, da = proj_net.dot_mult, proj_net.dot_add
    out = episode.cluster(proj_embds, conf.reshape(-1), NUM_IMAGES, dm, da, valid_threshold=None, sim_target='max')
    nov = ood.novelty_score(proj_embds, conf.reshape(-1), out['proto'], float(dm.detach()), float(da.detach()), 'max')
    # ---- the literal replica on the CPU, fed the MetaHead's outputs
    confs_c, activs_c = [t.cpu() for t in confs], [t.cpu() for t in activs]
    enc = [t.cpu() for t in (proj_net.anch_enc, proj_net.lev_enc, proj_net.cell_enc)]
    feed_r, conf_r, masks = ref.episode_feed(activs_c, confs_c, *enc, first_level=OFFSET)
    for s, m, c in zip(sel, masks, confs_c):
        assert m.sum(1).tolist() == [episode.kept_per_level(c.shape[2], c.shape[3])] * NUM_IMAGES      # no tie at a cut
        assert torch.equal(s.cpu().long(), ref.mask_indices(m))
    assert torch.equal(feed.cpu(), feed_r) and torch.equal(conf.cpu(), conf_r)
    w_ref = [m.weight.detach().cpu().clone().requires_grad_() for m in proj_net.projection if isinstance(m, torch.nn.Linear)]
    dots_ref = [dm.detach().cpu().clone().requires_grad_(), da.detach().cpu().clone().requires_grad_()]
    embds_r = om.projection_forward(w_ref, feed_r.reshape(-1, feed_r.shape[-1]))
    _close(proj_embds.detach(), embds_r.detach(), 'proj_embds')
    # decisions against the float64 form (exact where it decides clearly; a head with seeded random weights gives no separable
    # clusters, so no share of clear rows is asked for here - test_cluster_against_the_literal_form does that - but every row's pick
    # must still be within float32 resolution of the best); values against the literal float32 form on the same decisions
    sel_gpu = {k: out[k].cpu() for k in ('proto0', 'valid', 'proto', 'nearest')}
    lit = ref.cluster_literal(embds_r.detach(), conf_r.reshape(-1), dots_ref[0].detach(), dots_ref[1].detach(), NUM_IMAGES, None, 'max',
                              sel=sel_gpu)
    lean64 = ref.cluster_lean(embds_r.detach().double(), conf_r.reshape(-1).double(), 1.5, 0.25, NUM_IMAGES, None, 'max')
    _check_cluster(out, lit, lean64, 'max', nov, max_skipped=None)
    # ---- the differentiable remainder: same target, gradients (first and second order) as the replica's autograd
    weights = [m.weight for m in proj_net.projection if isinstance(m, torch.nn.Linear)]
    t = episode.target_from_selection(proj_embds, conf.reshape(-1), out, dm, da, 'max')
    for k in ('target_clust', 'sim', 'target', 'soft_thresh'):
        _close(t[k].detach(), out[k].cpu(), 'target_from_selection ' + k)
    logits = conf.reshape(-1)
    loss = _e2e_loss(t['target'], logits)
    g = torch.autograd.grad(loss, weights + [dm, da], create_graph=True)
    second = sum((gi * gi).sum() for gi in g[:2])
    g2 = torch.autograd.grad(second, weights)
    lit_g = ref.cluster_literal(embds_r, conf_r.reshape(-1), dots_ref[0], dots_ref[1], NUM_IMAGES, None, 'max', sel=sel_gpu)
    loss_r = _e2e_loss(lit_g['target'], conf_r.reshape(-1))
    assert abs(float(loss.detach()) - float(loss_r.detach())) <= 1e-4 * abs(float(loss_r.detach()))
    gr = torch.autograd.grad(loss_r, w_ref + dots_ref, create_graph=True)
    second_r = sum((gi * gi).sum() for gi in gr[:2])
    g2r = torch.autograd.grad(second_r, w_ref)
    for what, got, want in (('first order', g, gr), ('second order', g2, g2r)):
        scale = max(float(w.detach().abs().max()) for w in want)
        for i, (a, w) in enumerate(zip(got, want)):
            err = float((a.detach().cpu() - w.detach()).abs().max())
            print('%s gradient %d: max err %.3e, largest entry %.3e' % (what, i, err, scale))
            assert bool(torch.isfinite(a).all()) and scale > 0 and err <= 5e-3 * scale, (what, i, err, scale)


# ---- 6. graph capture ---------------------------------------------------------------------------------------------------------

def test_whole_chain_in_one_graph_replays_bit_for_bit():
    from ood_object_detection_amd import episode
    B, Fc, sides = 5, 64, [16, 8, 4]
    proj_net = _proj_net(Fc, width=128, seed=3)

    def chain(activs, confs):
        with torch.no_grad():
            sel = episode.select_anchors(confs)
            feed, conf = episode.projection_feed(activs, confs, sel, proj_net, first_level=OFFSET)
            embds = proj_net(feed).reshape(-1, 64)
            out = episode.cluster(embds, conf.reshape(-1), B, proj_net.dot_mult, proj_net.dot_add, valid_threshold=0.1)
        return [feed, conf, embds] + [out[k] for k in sorted(out)] + sel

    a1, c1 = _levels(31, B, Fc, sides)
    a2, c2 = _levels(32, B, Fc, sides)
    static_a = [t.clone(memory_format=torch.preserve_format) for t in a1]
    static_c = [t.clone(memory_format=torch.preserve_format) for t in c1]
    eager1 = [t.clone() for t in chain(a1, c1)]
    assert _same(eager1, chain(a1, c1))                                           # two eager runs are bit-identical
    eager2 = [t.clone() for t in chain(a2, c2)]
    assert not torch.equal(eager1[0], eager2[0])
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
