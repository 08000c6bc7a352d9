"""The projection phase's losses (infer.py:448-494) in torch: the literal form with its n x n `mask` / `sim_target` / `sim_mat`, as the
script writes it on the package's cosine_loss (pinned to the reference's fixture by tests/test_host.py), and the lean form of
rows and n x m products that stands in where the literal one cannot run.  Both take the discrete decisions (proto0, valid, proto,
nearest) as given, on whatever device / dtype their inputs have.  In the lean form a hinge is (1/n) sum_i a_i arg_i with the 0 / 1
vector `a` an argument (default arg_i >= 0, what clamp(min=0) passes), so the gradient is linear in `a`."""
import torch
import torch.nn.functional as F

import _episode_ref as eref

STAT_NAMES = ('task_obj_mean', 'task_obj_min', 'other_obj_mean', 'other_obj_max', 'no_obj_mean', 'no_obj_max')
LABEL_POOL = (-2, -1, -1, 0, 5, 5, 5, 9)
CLS_ID = 5


def group_stats(inner_target, labs, cls_id):
    """infer.py:474-491: -> (six statistics, NaN for an empty group; three counts)"""
    nan = torch.full((), float('nan'), dtype=inner_target.dtype)
    masks = (labs == cls_id, torch.logical_and(labs > -1, labs != cls_id), labs == -1)
    stats, counts = [], []
    for j, mk in enumerate(masks):
        sel = inner_target[mk]
        counts.append(int(mk.sum()))
        if counts[-1] == 0:
            stats += [nan, nan]
        else:
            stats += [sel.mean(), sel.min() if j == 0 else sel.max()]
    return dict(zip(STAT_NAMES, stats)), counts


def losses_literal(proj_embds, confs, labs, cls_id, sel, dot_mult, dot_add, sim_target='max', loss_mode='separate', margin=0.):
    """infer.py:423-494 with the decisions of `sel`"""
    from ood_object_detection_amd.effdet.loss import cosine_loss
    e = F.normalize(proj_embds, p=2)
    sim_mat = torch.matmul(e, e.t())
    soft_thresh = dot_mult * (confs + dot_add)
    soft_thresh_sig = soft_thresh.sigmoid()
    max_idxs0 = sel['proto0']
    valid = sel['valid']
    target_clust = sim_mat[:, max_idxs0[valid]].mean(1)
    max_idxs = sel['proto']
    target_clust = target_clust[max_idxs]
    proj_labs = labs
    zero = torch.zeros((), dtype=e.dtype)
    if sim_target == 'max':
        all_max_idxs = sel['nearest']
        all_max_sims_clust = torch.gather(sim_mat[:, max_idxs], 1, all_max_idxs.reshape(-1, 1)).reshape(-1)
        mask = torch.logical_and(proj_labs.view(-1, 1) == proj_labs.view(1, -1), proj_labs.view(1, -1) == cls_id)
        sim_t = torch.where(mask, 1., -1.).to(e.dtype)
        row_t = torch.gather(sim_t, 1, all_max_idxs.reshape(1, -1))
        if loss_mode == 'separate':
            clust_loss = cosine_loss(target_clust, sim_t[max_idxs, max_idxs], reduction='mean', margin=margin)
            embds_loss = cosine_loss(soft_thresh_sig * all_max_sims_clust, row_t, reduction='mean', margin=margin)
        elif loss_mode == 'same':
            clust_loss = zero
            embds_loss = cosine_loss(soft_thresh_sig * all_max_sims_clust * target_clust[all_max_idxs], row_t, reduction='mean', margin=margin)
        elif loss_mode == 'no_conf':
            clust_loss = cosine_loss(target_clust, sim_t[max_idxs, max_idxs], reduction='mean', margin=margin)
            embds_loss = cosine_loss(all_max_sims_clust, row_t, reduction='mean', margin=margin)
        else:
            raise ValueError(loss_mode)
        inner_target = soft_thresh_sig * target_clust[all_max_idxs] * all_max_sims_clust
        positives = int((row_t == 1.).sum())
    else:
        all_avg_sims_clust = sim_mat[:, max_idxs].mean(1)
        sim_t = torch.where(proj_labs.reshape(-1) == cls_id, 1., -1.).to(e.dtype)
        embds_loss = cosine_loss(soft_thresh_sig * all_avg_sims_clust, sim_t, reduction='mean', margin=margin)
        clust_loss = zero
        inner_target = soft_thresh_sig * all_avg_sims_clust
        positives = int((sim_t == 1.).sum())
    stats, counts = group_stats(inner_target.detach(), proj_labs.reshape(-1), cls_id)
    obj_target = (proj_labs > -1).to(e.dtype)
    obj_loss = F.binary_cross_entropy_with_logits(soft_thresh, obj_target, reduction='sum')
    return dict(clust_loss=clust_loss, embds_loss=embds_loss, obj_loss=obj_loss, inner_target=inner_target.detach(), stats=stats,
                counts=counts, positives=positives)


def losses_lean(proj_embds, confs, labs, cls_id, sel, dot_mult, dot_add, sim_target='max', loss_mode='separate', margin=0., a=None):
    """The same from row quantities and n x m products.  `a` [n]: the 0 / 1 weights of the embds hinge (None: arg >= 0).  Also
    returns the hinge arguments (`embds_arg` [n], `clust_arg` [m] or None) for the tests' kink bookkeeping."""
    e = F.normalize(proj_embds, p=2)
    n = e.shape[0]
    l = dot_mult * (confs + dot_add)
    s = l.sigmoid()
    valid = sel['valid']
    cmean = e[sel['proto0'][valid]].mean(0)
    P = e[sel['proto']]
    m = P.shape[0]
    target_clust = P @ cmean
    is_cls = labs == cls_id
    zero = torch.zeros((), dtype=e.dtype)
    clust_arg = None
    if sim_target == 'max':
        nearest = sel['nearest']
        sim = (e * P[nearest]).sum(1)
        t = torch.logical_and(is_cls[0], is_cls[nearest])           # row 0, column nearest_i (a value in [0, m)) of the n x n target
        x = {'separate': s * sim, 'same': s * sim * target_clust[nearest], 'no_conf': sim}[loss_mode]
        if loss_mode != 'same':
            y = is_cls[sel['proto']]
            clust_arg = torch.where(y, 1 - target_clust, target_clust - margin)
        inner_target = s * target_clust[nearest] * sim
    else:
        sim = e @ P.mean(0)
        t = is_cls
        x = s * sim
        inner_target = s * sim
    arg = torch.where(t, 1 - x, x - margin)
    if a is None:
        a = (arg.detach() >= 0).to(e.dtype)
    embds_loss = (a * arg).sum() / n
    clust_loss = ((clust_arg.detach() >= 0).to(e.dtype) * clust_arg).sum() / m if clust_arg is not None else zero
    tobj = (labs > -1).to(e.dtype)
    obj_loss = (l.clamp(min=0) - l * tobj + torch.log1p(torch.exp(-l.abs()))).sum()
    stats, counts = group_stats(inner_target.detach(), labs, cls_id)
    return dict(clust_loss=clust_loss, embds_loss=embds_loss, obj_loss=obj_loss, inner_target=inner_target.detach(), stats=stats,
                counts=counts, positives=int(t.sum()), embds_arg=arg.detach(), clust_arg=None if clust_arg is None else clust_arg.detach())


def draw_labels(seed, n, first_is_task, pool=LABEL_POOL):
    gen = torch.Generator().manual_seed(seed)
    labs = torch.tensor(pool, dtype=torch.int64)[torch.randint(0, len(pool), (n,), generator=gen)]
    labs[0] = CLS_ID if first_is_task else -1
    return labs


def decisions(x64, confs64, dot_mult, dot_add, num, sim_target):
    """the float64 lean `cluster_lean` decisions (and the full result, for decision_gaps)"""
    lean = eref.cluster_lean(x64, confs64, dot_mult, dot_add, num, None, sim_target)
    sel = {k: lean[k] for k in ('proto0', 'valid', 'proto')}
    sel['nearest'] = lean['nearest'] if sim_target == 'max' else torch.full((x64.shape[0],), -1, dtype=torch.int64)
    return sel, lean
