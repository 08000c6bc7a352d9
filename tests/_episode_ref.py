"""Literal restatements of infer.py's episode stage (projection phase :362-447, meta phase :566-654) in torch, as the script
writes them - they extend tests/test_infer_proj_gpu.py::_feed / _cluster with the quantile mask and the meta phase's validity rule -
and the lean form (no n x n matrix) that serves as the yardstick where the literal form cannot run.  Every function works on
whatever device / dtype its inputs have."""
import torch
import torch.nn.functional as F

NUM_ANCHS = 9


def quantile_mask(res_conf, map_h):
    """infer.py:380-386 / :584-589 without the tie loop (:387-390, which hard-codes 25 images): res_conf [B, N] -> bool [B, N]"""
    if map_h <= 4:
        return res_conf > -1000.
    q = torch.quantile(res_conf, 0.875, dim=1, keepdims=True)
    return res_conf > q


def tie_free(res_conf):
    """no two equal confidences in any image (then the mask keeps the same number of anchors in every image)"""
    s = torch.sort(res_conf, dim=1)[0]
    return bool((s[:, 1:] > s[:, :-1]).all())


def tie_free_confs(seed, B, N):
    """[B, N] float32 confidences in [-4, 4) without equal values inside an image: a random permutation of an even grid (normal
    samples of this many values do collide in float32)"""
    gen = torch.Generator().manual_seed(seed)
    perm = torch.stack([torch.randperm(N, generator=gen) for _ in range(B)])
    return perm.float() * (8.0 / N) - 4.0


def level_feed(level_embds_c, lev_confs_c, anch_enc, lev_enc_row, cell_enc_t):
    """infer.py:367-377 / :571-580: -> feed_embds [B, H W A, F + 42], res_conf [B, H W A]"""
    level_embds = level_embds_c.movedim(1, 3)
    lev_confs = lev_confs_c.movedim(1, 3).reshape(-1)
    B, H, W, Fc = level_embds.shape
    lev_enc = lev_enc_row.reshape(1, 1, -1).repeat(B, H, W, 1).reshape(-1, 6)
    cell_enc = cell_enc_t[:H].reshape(1, H, 1, 14).repeat(B, 1, W, 1)
    cell_enc = torch.cat([cell_enc, cell_enc.movedim(1, 2)], dim=2).reshape(-1, 14 * 2)
    flat_embds = level_embds.reshape(-1, Fc)
    anch = anch_enc.repeat(flat_embds.shape[0], 1)
    rep_embds = flat_embds.repeat_interleave(NUM_ANCHS, dim=0)
    lev_enc = lev_enc.repeat_interleave(NUM_ANCHS, dim=0)
    cell_enc = cell_enc.repeat_interleave(NUM_ANCHS, dim=0)
    feed_embds = torch.cat([rep_embds, anch, lev_enc, cell_enc], dim=1)
    return feed_embds.reshape(B, -1, feed_embds.shape[-1]), lev_confs.reshape(B, -1)


def episode_feed(obj_embds, class_out, anch_enc, lev_enc_t, cell_enc_t, first_level=0, masks=None):
    """infer.py:366-420 / :570-609: -> proj_feed [B, R, F + 42], confs [B, R], masks (per level bool [B, N]).  `masks` given: used
    instead of the quantile masks."""
    feeds, confs, used = [], [], []
    for level_ix, (e, c) in enumerate(zip(obj_embds, class_out)):
        feed_embds, res_conf = level_feed(e, c, anch_enc, lev_enc_t[first_level + level_ix], cell_enc_t)
        B = res_conf.shape[0]
        mask = masks[level_ix] if masks is not None else quantile_mask(res_conf, c.shape[2])
        used.append(mask)
        confs.append(res_conf[mask].reshape(B, -1))
        feeds.append(feed_embds[mask].reshape(B, -1, feed_embds.shape[-1]))
    return torch.cat(feeds, dim=1), torch.cat(confs, dim=1), used


def mask_indices(mask):
    """bool [B, N] with equally many set per row -> int64 [B, keep] ascending"""
    B = mask.shape[0]
    return mask.nonzero()[:, 1].reshape(B, -1)


def cluster_literal(proj_embds, confs, dot_mult, dot_add, num, valid_threshold=None, sim_target='max', sel=None):
    """infer.py:423-472 (valid_threshold None) / :607-652 (a float), n x n matrices and all.  `sel` (a dict with proto0, valid,
    proto, nearest) replaces the discrete decisions, as tests/test_infer_proj_gpu.py::_cluster does."""
    proj_embds = F.normalize(proj_embds, p=2)
    sim_mat = torch.matmul(proj_embds, proj_embds.t())
    soft_thresh = (dot_mult * (confs + dot_add)).sigmoid()
    thresh_mat = torch.matmul(soft_thresh.reshape(-1, 1), soft_thresh.reshape(1, -1))
    weighted_sim = (thresh_mat * sim_mat).reshape(num, -1, sim_mat.shape[0])
    img_avg_sims_all = weighted_sim.mean(2)
    arange = torch.arange(0, sim_mat.shape[0], weighted_sim.shape[1], device=sim_mat.device)
    max_idxs = torch.argmax(img_avg_sims_all, dim=1) + arange if sel is None else sel['proto0'].to(arange.device)
    proto0 = max_idxs
    init_cluster = sim_mat[max_idxs][:, max_idxs]
    avg_init0 = init_cluster.mean(1) - 1. / num
    if sel is not None:
        valid = sel['valid'].to(arange.device)
    elif valid_threshold is None:
        valid = avg_init0 > avg_init0.mean()                                       # :438
    else:
        valid = avg_init0 > valid_threshold                                        # :631
    target_clust = sim_mat[:, max_idxs[valid]].mean(1)
    if valid_threshold is None:
        img_avg_sims_clust = weighted_sim[:, :, max_idxs[valid]].mean(2)           # :441
    else:
        img_avg_sims_clust = weighted_sim[:, :, max_idxs[valid]].sum(2)            # :635
    max_idxs = torch.max(img_avg_sims_clust, dim=1)[1] + arange if sel is None else sel['proto'].to(arange.device)
    target_clust = target_clust[max_idxs]
    init_cluster = sim_mat[max_idxs][:, max_idxs]
    avg_init = init_cluster.mean(1) - 1. / num
    cols = sim_mat[:, max_idxs]
    out = dict(soft_thresh=soft_thresh, proto0=proto0, avg_init0=avg_init0, valid=valid, proto=max_idxs, avg_init=avg_init,
               target_clust=target_clust)
    if sim_target == 'max':
        if sel is None:
            sim, nearest = torch.max(cols, dim=1)                                  # :449 / :646
        else:
            nearest = sel['nearest'].to(arange.device)
            sim = torch.gather(cols, 1, nearest.reshape(-1, 1)).reshape(-1)
        out.update(sim=sim, nearest=nearest, target=(soft_thresh * target_clust[nearest] * sim).reshape(-1))    # :465 / :648
    else:
        sim = cols.mean(1)                                                         # :467 / :650
        out.update(sim=sim, target=soft_thresh * sim)                              # :472 / :652
    return out


def cluster_lean(proj_embds, confs, dot_mult, dot_add, num, valid_threshold=None, sim_target='max'):
    """The same quantities from rank-1 / n x m products only.  With e the normalised rows, s the soft threshold, g = sum_j s_j e_j:
    weighted_sim.mean(2)[i] = s_i (e_i . g) / n;  sim_mat[:, Pv].mean(1)[i] = e_i . mean_v e_pv;
    weighted_sim[:, :, Pv].sum(2)[i] = s_i (e_i . sum_v s_pv e_pv).  Also returns what the decisions were taken on (score0, score1
    [num, rows], thr, cols [n, num]) for `decision_gaps`."""
    e = F.normalize(proj_embds, p=2)
    n = e.shape[0]
    p = n // num
    s = (dot_mult * (confs + dot_add)).sigmoid()
    g = (s[:, None] * e).sum(0)
    score0 = (s * (e @ g) / n).reshape(num, p)
    arange = torch.arange(0, n, p, device=e.device)
    proto0 = torch.argmax(score0, dim=1) + arange
    avg_init0 = (e[proto0] @ e[proto0].t()).mean(1) - 1. / num
    thr = avg_init0.mean() if valid_threshold is None else torch.as_tensor(valid_threshold, dtype=e.dtype, device=e.device)
    valid = avg_init0 > thr
    pv = proto0[valid]
    target_all = e @ e[pv].mean(0)
    score1 = (s * (e @ (s[pv, None] * e[pv]).sum(0))).reshape(num, p)
    if valid_threshold is None:
        score1 = score1 / max(int(valid.sum()), 1)
    proto = torch.argmax(score1, dim=1) + arange
    target_clust = target_all[proto]
    avg_init = (e[proto] @ e[proto].t()).mean(1) - 1. / num
    cols = e @ e[proto].t()
    out = dict(soft_thresh=s, proto0=proto0, avg_init0=avg_init0, valid=valid, proto=proto, avg_init=avg_init,
               target_clust=target_clust, score0=score0, score1=score1, thr=thr, cols=cols)
    if sim_target == 'max':
        sim, nearest = torch.max(cols, dim=1)
        out.update(sim=sim, nearest=nearest, target=s * target_clust[nearest] * sim)
    else:
        sim = cols.mean(1)
        out.update(sim=sim, target=s * sim)
    return out


def decision_gaps(lean):
    """From a (float64) cluster_lean result: the smallest per-image top-2 gap of either pick relative to max|score|, the smallest
    validity margin |avg_init0 - threshold|, and per row the gap between its two most similar prototypes."""
    rel = []
    for sc in (lean['score0'], lean['score1']):
        top = torch.topk(sc, 2, dim=1)[0]
        rel.append(float((top[:, 0] - top[:, 1]).min() / sc.abs().max()))
    margin = float((lean['avg_init0'] - lean['thr']).abs().min())
    if lean['cols'].shape[1] > 1:
        top = torch.topk(lean['cols'], 2, dim=1)[0]
        row_gap = top[:, 0] - top[:, 1]
    else:
        row_gap = torch.full_like(lean['cols'][:, 0], float('inf'))
    return min(rel), margin, row_gap


def clustered_rows(seed, num, rows, d):
    """three cluster centres plus 0.7 x normal noise; confs 2 N(0, 1) - 3 (float32, CPU)"""
    gen = torch.Generator().manual_seed(seed)
    centres = torch.randn(3, d, generator=gen)
    which = torch.randint(0, 3, (num * rows,), generator=gen)
    x = centres[which] + 0.7 * torch.randn(num * rows, d, generator=gen)
    confs = 2. * torch.randn(num * rows, generator=gen) - 3.
    return x, confs
