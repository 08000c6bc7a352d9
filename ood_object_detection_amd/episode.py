"""The few-shot episode stage between the MetaHead's outputs and `ood.novelty_score` (infer.py:362-447 projection phase,
:566-654 meta phase) on the HIP kernels of csrc/episode.hip and csrc/episode_loss.hip:

    sel = select_anchors(confs)                                   # the anchors above the 0.875 confidence quantile, per level and image
    feed, conf = projection_feed(activs, confs, sel, proj_net)    # [embedding | anchor enc | level enc | cell enc] rows
    out = cluster(proj_net(feed).reshape(-1, d), conf.reshape(-1), B, dot_mult, dot_add)
    t = target_from_selection(proj_embds, conf.reshape(-1), out, dot_mult, dot_add)     # the same target, with autograd history
    loss = projection_losses(proj_embds, conf.reshape(-1), labs, cls_id, out, dot_mult, dot_add)   # infer.py:448-498, forward and backward
    supp = support_loss(proj_embds, conf.reshape(-1), cls_logits, out, dot_mult, dot_add)          # infer.py:645-658, differentiable twice
    fast = inner_update(class_net.named_parameters(), inner_grad, learnable_lr)                    # infer.py:660-678, learnable step sizes

float32 GPU tensors only, no CPU fallback.  Nothing here synchronises with the host and no allocation depends on a device value,
so the whole chain can be captured in one `torch.cuda.graph`.  The n x n matrices of the script (`sim_mat`, `thresh_mat`,
`weighted_sim`, `mask`, `sim_target`) are never formed: every use of them is rank-1 or n x m (see csrc/episode.hip,
csrc/episode_loss.hip and csrc/episode_support.hip; the inner update is csrc/inner_update.hip)."""
import ctypes

import torch
import torch.nn.functional as F

from . import _lib

QUANTILE_NUM, QUANTILE_DEN = 7, 8          # 0.875 (infer.py:385 / :588)


def kept_per_level(h: int, w: int, num_anchors: int = 9) -> int:
    """Anchors per image the episode code keeps on an h x w level: all of them when h <= 4 (infer.py:381-382), else what
    `res_conf > torch.quantile(res_conf, 0.875)` keeps on tie-free data, N - 1 - floor(0.875 (N - 1))."""
    n = int(num_anchors) * int(h) * int(w)
    if h <= 4:
        return n
    return n - 1 - (QUANTILE_NUM * (n - 1)) // QUANTILE_DEN


def _check(t, dim, what):
    if not torch.is_tensor(t) or t.device.type != 'cuda' or t.dtype != torch.float32 or t.dim() != dim:
        raise RuntimeError('%s: expected a float32 %d-d GPU tensor (no CPU fallback)' % (what, dim))


def _use_max(sim_target):
    if sim_target not in ('avg', 'max'):
        raise ValueError("sim_target must be 'avg' or 'max' (infer.py FLAGS.sim_target)")
    return 1 if sim_target == 'max' else 0


def _check_vector(t, dev, dtype, n, what, name):
    if not torch.is_tensor(t) or t.device != dev or t.dtype != dtype or t.numel() != n:
        raise RuntimeError('%s: %s must be a %s GPU tensor of %d elements (no CPU fallback)' % (what, name, dtype, n))


def _flat(t, n):
    return t.detach().reshape(n).contiguous()


def _workspace(query, n, d, m, dev, limits):
    """the float32 workspace the kernels of an (n, d, m) problem ask for; ValueError(limits) when they do not take the shape"""
    ws_floats = query(n, d, m) if n > 0 and m > 0 else -1
    if ws_floats < 0:
        raise ValueError(limits)
    return torch.empty(ws_floats, dtype=torch.float32, device=dev), ws_floats


LOSS_LIMITS = 'need n >= num prototypes, at most 64 prototypes, d <= 512 and prototypes * d <= 16384'


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _nhwc(t):
    """[B, C, H, W] -> (tensor that owns [B, H, W, C] memory, image stride); the MetaHead's permuted views are taken as they are"""
    B, C, H, W = t.shape
    v = t.detach().permute(0, 2, 3, 1)
    if not (v.stride(3) == 1 and v.stride(2) == C and v.stride(1) == W * C and (B == 1 or v.stride(0) >= H * W * C)):
        v = v.contiguous()
    return v, (v.stride(0) if B > 1 else H * W * C)


def _ptrs(vals):
    return (ctypes.c_void_p * len(vals))(*vals)


def _lls(vals):
    return (ctypes.c_longlong * len(vals))(*vals)


def _ints(vals):
    return (ctypes.c_int * len(vals))(*vals)


def select_anchors(confs):
    """confs[l] [B, A, H, W] (the MetaHead's outputs, views of [B, H, W, A] memory are not copied) -> per level int32
    [B, kept_per_level(H, W, A)]: the kept anchors' indices in (y, x, a) order, ascending - the order boolean-mask indexing with
    the reference's `res_conf > quantile` mask gives, and on tie-free data the same set.  Equal confidences at the cut resolve to
    the lower index (the project's top-k convention), so every image keeps exactly kept_per_level anchors.  The reference's tie
    loop (infer.py:387-390) hard-codes 25 images and never terminates otherwise; it is not reproduced."""
    if not confs or len(confs) > 8:
        raise ValueError('between 1 and 8 levels')
    lib = _lib.load()
    keepalive, ptr, stride, count, keep, outs = [], [], [], [], [], []
    B = confs[0].shape[0]
    for c in confs:
        _check(c, 4, 'select_anchors')
        if c.shape[0] != B:
            raise ValueError('levels disagree on the batch size')
        v, s = _nhwc(c)
        _, A, H, W = c.shape
        keepalive.append(v)
        ptr.append(v.data_ptr()); stride.append(s); count.append(A * H * W); keep.append(kept_per_level(H, W, A))
        outs.append(torch.empty(B, keep[-1], dtype=torch.int32, device=c.device))
    st = _stream(confs[0].device)
    _lib.check(lib.effdet_episode_select(st, B, len(confs), _ptrs(ptr), _lls(stride), _ints(count), _ints(keep),
                                         _ptrs([o.data_ptr() for o in outs])), 'effdet_episode_select')
    return outs


def projection_feed(activs, confs, sel, proj_net, first_level=0):
    """-> (feed [B, R, F + 42], conf [B, R]), R = sum of the kept anchors over the levels, concatenated per image as infer.py:418 /
    :606 do.  A feed row is [F embedding | anch_enc[a] (8) | lev_enc[first_level + l] (6) | cell enc (28)] (:366-378), copied
    bit for bit; `first_level` is 0 in the projection phase and supp_level_offset in the meta phase.  activs[l] [B, F, H, W] and
    confs[l] [B, A, H, W] are the MetaHead's outputs (ret_activs=True), sel the result of select_anchors; square maps of at most
    80 cells a side.  Both results are copies without autograd history (FLAGS.proj_stop_grad).  `feed` is a view of a zero-padded [B, R, ceil8(F + 42)] buffer that ProjectionNet's inference path consumes
    without its re-pack copy."""
    nl = len(confs)
    if nl == 0 or nl > 8 or len(activs) != nl or len(sel) != nl:
        raise ValueError('activs, confs and sel must list the same 1 to 8 levels')
    lib = _lib.load()
    dev = confs[0].device
    B, A = confs[0].shape[:2]
    Fc = activs[0].shape[1]
    anch, lev, cell = (t.detach().to(device=dev, dtype=torch.float32).contiguous() for t in (proj_net.anch_enc, proj_net.lev_enc, proj_net.cell_enc))
    if A > anch.shape[0] or anch.shape[1] != 8 or lev.shape[1] != 6 or cell.shape[1] != 14:
        raise ValueError('unexpected encoding tables')
    if first_level < 0 or first_level + nl > lev.shape[0]:
        raise ValueError('level encodings exist for levels 0 .. %d' % (lev.shape[0] - 1))
    keepalive, aptr, astr, cptr, cstr, sptr, keeps, widths = [], [], [], [], [], [], [], []
    for a, c, s in zip(activs, confs, sel):
        _check(a, 4, 'projection_feed'); _check(c, 4, 'projection_feed')
        H, W = c.shape[2:]
        if H != W or H > cell.shape[0] or a.shape != (B, Fc, H, W) or c.shape[:2] != (B, A):
            raise ValueError('square maps of at most %d cells a side, one batch size and width for all levels' % cell.shape[0])
        if s.device != dev or s.dtype != torch.int32 or s.dim() != 2 or s.shape[0] != B or s.shape[1] > A * H * W or s.shape[1] == 0:
            raise ValueError('sel[l] must be the int32 [B, keep] GPU tensor select_anchors returns')
        av, ast = _nhwc(a)
        cv, cst = _nhwc(c)
        sv = s.contiguous()
        keepalive += [av, cv, sv]
        aptr.append(av.data_ptr()); astr.append(ast); cptr.append(cv.data_ptr()); cstr.append(cst)
        sptr.append(sv.data_ptr()); keeps.append(sv.shape[1]); widths.append(W)
    R, K = sum(keeps), Fc + 42
    Kp = (K + 7) // 8 * 8
    feed = torch.empty(B, R, Kp, dtype=torch.float32, device=dev)
    conf = torch.empty(B, R, dtype=torch.float32, device=dev)
    st = _stream(dev)
    _lib.check(lib.effdet_episode_feed(st, B, nl, _ptrs(aptr), _lls(astr), _ptrs(cptr), _lls(cstr), _ptrs(sptr), _ints(keeps),
                                       _ints(widths), anch.data_ptr(), lev.data_ptr(), lev.shape[0], cell.data_ptr(), cell.shape[0],
                                       int(first_level), A, Fc, Kp, feed.data_ptr(), conf.data_ptr()), 'effdet_episode_feed')
    view = feed[..., :K]
    view._effdet_zero_tail = True            # ProjectionNet.forward: the row pitch is ceil8(K) and the tail is zero
    return view, conf


def _dots(dot_mult, dot_add, dev):
    """Python numbers travel by value; tensors (proj_net.dot_mult / dot_add) stay on the device, so nothing synchronises"""
    if torch.is_tensor(dot_mult) or torch.is_tensor(dot_add):
        pair = [torch.as_tensor(v).detach().to(device=dev, dtype=torch.float32).reshape(()) for v in (dot_mult, dot_add)]
        return 0.0, 0.0, torch.stack(pair).contiguous()
    return float(dot_mult), float(dot_add), None


def cluster(proj_embds, confs, num_images, dot_mult, dot_add, valid_threshold=None, sim_target='max'):
    """infer.py:423-447 (valid_threshold=None: `valid = avg_init > avg_init.mean()`, :438) / :605-654 (a float: `avg_init >
    FLAGS.sim_thresh`, :631).  proj_embds [n, d] un-normalised ProjectionNet outputs, n = num_images * rows, confs [n] logits;
    dot_mult / dot_add numbers or (GPU) tensors.  Returns dict(soft_thresh [n]; proto0 [m] int64 (first `max_idxs`), avg_init0 [m];
    valid [m] bool, n_valid [1] int32; proto [m] int64 (second `max_idxs`), avg_init [m], target_clust [m]; sim [n]
    (`all_max_sims_clust`, or the mean for 'avg'); nearest [n] int64 (`all_max_idxs`; -1 for 'avg'); target [n] (:648 / :652)).
    An empty valid set gives NaN target_clust / target as in the reference; n_valid says so.  argmax ties go to the lower index.
    num_images <= 64, d <= 512, num_images * d <= 16384."""
    _check(proj_embds, 2, 'cluster')
    use_max = _use_max(sim_target)
    lib = _lib.load()
    e = proj_embds.detach().contiguous()
    n, d = e.shape
    m = int(num_images)
    dev = e.device
    _check_vector(confs, dev, torch.float32, n, 'cluster', 'confs')
    c = _flat(confs, n)
    ws, ws_floats = _workspace(lib.effdet_episode_cluster_workspace_floats, n, d, m, dev,
                               'need n % num_images == 0, num_images <= 64, d <= 512 and num_images * d <= 16384')
    dm, da, dots = _dots(dot_mult, dot_add, dev)
    fn = torch.empty(4, n, dtype=torch.float32, device=dev)              # soft_thresh, sim, target, (spare)
    fm = torch.empty(3, m, dtype=torch.float32, device=dev)              # avg_init0, avg_init, target_clust
    im = torch.empty(2, m, dtype=torch.int64, device=dev)
    nearest = torch.empty(n, dtype=torch.int64, device=dev)
    valid = torch.empty(m, dtype=torch.bool, device=dev)
    n_valid = torch.empty(1, dtype=torch.int32, device=dev)
    st = _stream(dev)
    _lib.check(lib.effdet_episode_cluster(st, e.data_ptr(), c.data_ptr(), n, d, m, dm, da, dots.data_ptr() if dots is not None else None,
                                          0 if valid_threshold is None else 1, 0.0 if valid_threshold is None else float(valid_threshold),
                                          use_max, ws.data_ptr(), ws_floats, fn[0].data_ptr(), im[0].data_ptr(),
                                          fm[0].data_ptr(), valid.data_ptr(), n_valid.data_ptr(), im[1].data_ptr(), fm[1].data_ptr(),
                                          fm[2].data_ptr(), fn[1].data_ptr(), nearest.data_ptr(), fn[2].data_ptr()),
               'effdet_episode_cluster')
    return {'soft_thresh': fn[0], 'proto0': im[0], 'avg_init0': fm[0], 'valid': valid, 'n_valid': n_valid, 'proto': im[1],
            'avg_init': fm[1], 'target_clust': fm[2], 'sim': fn[1], 'nearest': nearest, 'target': fn[2]}


def target_from_selection(proj_embds, confs, out, dot_mult, dot_add, sim_target='max'):
    """The differentiable remainder: `target_clust`, `sim` and `target` re-derived from the indices `cluster` returned, as plain
    torch row gathers and row dot products on [n, d] (no n x n), so training code gets them with autograd history, also under
    create_graph=True.  The discrete decisions (prototypes, valid set, nearest prototype) are constants here, as they are
    non-differentiable in the reference.  Returns dict(soft_thresh, target_clust [m], sim [n], target [n]).  The meta phase's
    binary cross-entropy on this target has its own HIP kernels at both orders: `support_loss`."""
    _check(proj_embds, 2, 'target_from_selection')
    use_max = _use_max(sim_target)
    e = F.normalize(proj_embds, p=2)
    soft_thresh = (dot_mult * (confs.reshape(-1) + dot_add)).sigmoid()
    valid = out['valid'].to(e.dtype)
    cmean = (e[out['proto0']] * valid[:, None]).sum(0) / valid.sum()      # mean of the valid first prototypes (NaN when none is)
    protos = e[out['proto']]
    target_clust = protos @ cmean
    if use_max:
        nearest = out['nearest']
        sim = (e * protos[nearest]).sum(1)
        target = soft_thresh * target_clust[nearest] * sim
    else:
        sim = e @ protos.mean(0)
        target = soft_thresh * sim
    return {'soft_thresh': soft_thresh, 'target_clust': target_clust, 'sim': sim, 'target': target}


LOSS_MODES = {'separate': 0, 'same': 1, 'no_conf': 2}       # infer.py FLAGS.loss_mode
STAT_NAMES = ('task_obj_mean', 'task_obj_min', 'other_obj_mean', 'other_obj_max', 'no_obj_mean', 'no_obj_max')


def _proj_loss_args(e, c, labs, cls, dots, idx, n, d, m, use_max, mode, margin, dm, da):
    return (e.data_ptr(), c.data_ptr(), labs.data_ptr(), n, d, m, cls[0], cls[1].data_ptr() if cls[1] is not None else None, dm, da,
            dots.data_ptr() if dots is not None else None, idx[0].data_ptr(), idx[1].data_ptr(), idx[2].data_ptr(),
            idx[3].data_ptr() if idx[3] is not None else None, use_max, mode, margin)


class _ProjectionLosses(torch.autograd.Function):
    """effdet_episode_proj_loss / _backward: first order only (the projection phase calls final_loss.backward(), infer.py:787-789)"""

    @staticmethod
    def forward(ctx, proj_embds, confs, dot_mult, dot_add, labs, cls, idx, m, use_max, mode, margin):
        lib = _lib.load()
        e = proj_embds.detach().contiguous()
        n, d = e.shape
        dev = e.device
        c = _flat(confs, n)
        ws, ws_floats = _workspace(lib.effdet_episode_proj_loss_workspace_floats, n, d, m, dev, LOSS_LIMITS)
        dm, da, dots = _dots(dot_mult, dot_add, dev)
        losses = torch.empty(3, dtype=torch.float32, device=dev)
        inner = torch.empty(n, dtype=torch.float32, device=dev)
        stats = torch.empty(6, dtype=torch.float32, device=dev)
        counts = torch.empty(3, dtype=torch.int32, device=dev)
        args = _proj_loss_args(e, c, labs, cls, dots, idx, n, d, m, use_max, mode, margin, dm, da)
        _lib.check(lib.effdet_episode_proj_loss(_stream(dev), *args, ws.data_ptr(), ws_floats, losses.data_ptr(), inner.data_ptr(), stats.data_ptr(),
                                                counts.data_ptr()), 'effdet_episode_proj_loss')
        ctx.keep = (e, c, labs, cls, dots, idx, ws)
        ctx.scalars = (n, d, m, use_max, mode, margin, dm, da, ws_floats)
        ctx.shapes = (proj_embds.shape, confs.shape, tuple(t.shape if torch.is_tensor(t) else None for t in (dot_mult, dot_add)))
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(inner, stats, counts)
        return losses[0], losses[1], losses[2], inner, stats, counts

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_clust, g_embds, g_obj, *_):
        lib = _lib.load()
        e, c, labs, cls, dots, idx, ws = ctx.keep
        n, d, m, use_max, mode, margin, dm, da, ws_floats = ctx.scalars
        dev = e.device
        zero = torch.zeros((), dtype=torch.float32, device=dev)
        gup = torch.stack([zero if g is None else g.detach().to(dtype=torch.float32).reshape(()) for g in (g_clust, g_embds, g_obj)])
        d_e = torch.empty(n, d, dtype=torch.float32, device=dev)
        d_c = torch.empty(n, dtype=torch.float32, device=dev)
        d_dots = torch.empty(2, dtype=torch.float32, device=dev)
        args = _proj_loss_args(e, c, labs, cls, dots, idx, n, d, m, use_max, mode, margin, dm, da)
        _lib.check(lib.effdet_episode_proj_loss_backward(_stream(dev), *args, gup.data_ptr(), ws.data_ptr(), ws_floats, d_e.data_ptr(), d_c.data_ptr(),
                                                         d_dots.data_ptr()), 'effdet_episode_proj_loss_backward')
        e_shape, c_shape, dot_shapes = ctx.shapes
        g_dots = [d_dots[i].reshape(s) if s is not None and ctx.needs_input_grad[2 + i] else None for i, s in enumerate(dot_shapes)]
        return (d_e.reshape(e_shape), d_c.reshape(c_shape), g_dots[0], g_dots[1]) + (None,) * 7


def projection_losses(proj_embds, confs, labs, cls_id, sel, dot_mult, dot_add, sim_target='max', loss_mode='separate', margin=0.):
    """infer.py:448-498: the losses the projection phase trains on, from the decisions `cluster` took, on the HIP kernels of
    csrc/episode_loss.hip - no n x n `mask` / `sim_target` / `sim_mat`, forward or backward.  proj_embds [n, d] un-normalised
    ProjectionNet outputs, confs [n] logits, labs [n] int64 anchor labels (-2 / -1 / class ids) after the same selection, cls_id
    the task class (a number, or a tensor, which is read on the device), dot_mult / dot_add numbers or tensors.  `sel` is the
    dict `cluster` returns; only proto0, valid, proto, nearest are read, so a caller may supply its own decisions (indices outside
    their range are clamped into it by the kernels).  loss_mode 'separate' / 'same' / 'no_conf' applies to sim_target 'max'.
    `torch.gather(sim_target, 1, all_max_idxs.reshape(1, -1))` of the script reads row 0 and column nearest_i of the n x n
    target, so a row's target is +1 iff labs[0] == cls_id and labs[nearest_i] == cls_id with nearest_i in [0, m): reproduced.
    Returns dict(clust_loss, embds_loss, obj_loss: 0-d, with autograd history to proj_embds, confs and to dot_mult / dot_add
    when they are tensors that require grad; inner_target [n] (detached); stats: task_obj_mean, task_obj_min, other_obj_mean,
    other_obj_max, no_obj_mean, no_obj_max as device scalars, NaN for an empty group; counts [3] int32: the three group sizes).
    The backward is once-differentiable: the projection phase is first order (infer.py:787-789).  The meta phase differentiates
    its loss twice; that is `support_loss`.  With nothing requiring grad only the forward runs.  An empty
    valid set gives NaN clust_loss (and NaN 'same' embds_loss / inner_target) as the reference does; obj_loss stays finite."""
    use_max = _use_max(sim_target)
    if loss_mode not in LOSS_MODES:
        raise ValueError("loss_mode must be 'separate', 'same' or 'no_conf' (infer.py FLAGS.loss_mode)")
    _check(proj_embds, 2, 'projection_losses')
    n = proj_embds.shape[0]
    dev = proj_embds.device
    _check_vector(confs, dev, torch.float32, n, 'projection_losses', 'confs')
    _check_vector(labs, dev, torch.int64, n, 'projection_losses', 'labs')
    m, idx = _sel_indices(sel, dev, n, use_max, 'projection_losses')
    if torch.is_tensor(cls_id):
        cls = (0, cls_id.detach().to(device=dev, dtype=torch.int64).reshape(1))
    else:
        cls = (int(cls_id), None)
    out = _ProjectionLosses.apply(proj_embds, confs, dot_mult, dot_add, _flat(labs, n), cls, idx, m, use_max, LOSS_MODES[loss_mode], float(margin))
    return {'clust_loss': out[0], 'embds_loss': out[1], 'obj_loss': out[2], 'inner_target': out[3],
            'stats': dict(zip(STAT_NAMES, out[4].unbind(0))), 'counts': out[5]}


def _sel_indices(sel, dev, n, use_max, what):
    m = int(sel['proto'].numel())
    idx = []
    for key, dtype, count in (('proto0', torch.int64, m), ('valid', torch.bool, m), ('proto', torch.int64, m), ('nearest', torch.int64, n)):
        if key == 'nearest' and not use_max:
            idx.append(None)
            continue
        _check_vector(sel[key], dev, dtype, count, what, 'sel[%r]' % key)
        idx.append(_flat(sel[key], count))
    return m, tuple(idx)


class _SuppState:
    """what the three passes of one support_loss call share: detached inputs, decisions, the workspace the forward filled"""

    def args(self, thresh=None):
        e, c, x, idx, dots = self.e, self.c, self.x, self.idx, self.dots
        a = (e.data_ptr(), c.data_ptr(), x.data_ptr(), self.n, self.d, self.m, self.dm, self.da, dots.data_ptr() if dots is not None else None,
             idx[0].data_ptr(), idx[1].data_ptr(), idx[2].data_ptr(), idx[3].data_ptr() if idx[3] is not None else None, self.use_max)
        return a if thresh is None else a + (thresh,)


def _opt(t, shape):
    """a cotangent or None -> (float32 contiguous tensor of `shape` or None, its pointer or None)"""
    if t is None:
        return None, None
    t = t.detach().to(dtype=torch.float32).expand(shape).contiguous()
    return t, t.data_ptr()


class _SupportLoss(torch.autograd.Function):
    """effdet_episode_supp_loss; its backward is _SupportLossGrad, itself differentiable once"""

    @staticmethod
    def forward(ctx, proj_embds, confs, logits, dot_mult, dot_add, idx, m, use_max, thresh_grad):
        lib = _lib.load()
        st = _SuppState()
        st.e = proj_embds.detach().contiguous()
        st.n, st.d = st.e.shape
        dev = st.e.device
        st.c, st.x = _flat(confs, st.n), _flat(logits, st.n)
        st.idx, st.m, st.use_max, st.thresh_grad = idx, m, use_max, thresh_grad
        st.ws, st.ws_floats = _workspace(lib.effdet_episode_supp_loss_workspace_floats, st.n, st.d, m, dev, LOSS_LIMITS)
        st.dm, st.da, st.dots = _dots(dot_mult, dot_add, dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        target = torch.empty(st.n, dtype=torch.float32, device=dev)
        _lib.check(lib.effdet_episode_supp_loss(_stream(dev), *st.args(), st.ws.data_ptr(), st.ws_floats,
                                                loss.data_ptr(), target.data_ptr()), 'effdet_episode_supp_loss')
        ctx.st = st
        ctx.dot_tensors = tuple(torch.is_tensor(t) for t in (dot_mult, dot_add))
        ctx.save_for_backward(proj_embds, confs, logits, *(t for t in (dot_mult, dot_add) if torch.is_tensor(t)))
        ctx.mark_non_differentiable(target)
        return loss, target

    @staticmethod
    def backward(ctx, g, _):
        saved = list(ctx.saved_tensors)
        proj_embds, confs, logits = saved[:3]
        rest = saved[3:]
        dot_mult, dot_add = (rest.pop(0) if is_t else None for is_t in ctx.dot_tensors)
        d_e, d_c, d_x, d_m, d_a = _SupportLossGrad.apply(g, proj_embds, confs, logits, dot_mult, dot_add, ctx.st)
        if not ctx.st.thresh_grad:
            d_c = d_m = d_a = None                      # soft_thresh is a constant: nothing reaches confs or the dots through it
        return (d_e, d_c, d_x, d_m if ctx.dot_tensors[0] else None, d_a if ctx.dot_tensors[1] else None, None, None, None, None)


class _SupportLossGrad(torch.autograd.Function):
    """effdet_episode_supp_loss_backward, with effdet_episode_supp_loss_backward2 as its (once-differentiable) backward"""

    @staticmethod
    def forward(ctx, g, proj_embds, confs, logits, dot_mult, dot_add, st):
        lib = _lib.load()
        dev = st.e.device
        gup = g.detach().to(dtype=torch.float32).reshape(1).contiguous()
        d_e = torch.empty(st.n, st.d, dtype=torch.float32, device=dev)
        d_cx = torch.empty(2, st.n, dtype=torch.float32, device=dev)
        d_dots = torch.empty(2, dtype=torch.float32, device=dev)
        _lib.check(lib.effdet_episode_supp_loss_backward(_stream(dev), *st.args(1 if st.thresh_grad else 0),
                                                         gup.data_ptr(), st.ws.data_ptr(), st.ws_floats, d_e.data_ptr(), d_cx[0].data_ptr(),
                                                         d_cx[1].data_ptr(), d_dots.data_ptr()), 'effdet_episode_supp_loss_backward')
        ctx.st, ctx.gup = st, gup
        ctx.save_for_backward(proj_embds, confs, logits)     # the kernels read st's aliases; saved so that an in-place change raises
        ctx.shapes = (g.shape, proj_embds.shape, confs.shape, logits.shape) + tuple(t.shape if torch.is_tensor(t) else None for t in (dot_mult, dot_add))
        ctx.set_materialize_grads(False)
        return (d_e.reshape(proj_embds.shape), d_cx[0].reshape(confs.shape), d_cx[1].reshape(logits.shape),
                d_dots[0].reshape(ctx.shapes[4] or ()), d_dots[1].reshape(ctx.shapes[5] or ()))

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, v_e, v_c, v_x, v_m, v_a):
        lib = _lib.load()
        st = ctx.st
        ctx.saved_tensors                                    # autograd's version check of the inputs st aliases
        dev = st.e.device
        keep = [_opt(v_e, (st.n, st.d)), _opt(None if v_c is None else v_c.reshape(-1), (st.n,)),
                _opt(None if v_x is None else v_x.reshape(-1), (st.n,)), _opt(None if v_m is None else v_m.reshape(()), ()), _opt(None if v_a is None else v_a.reshape(()), ())]
        d_g = torch.empty(1, dtype=torch.float32, device=dev)
        h_e = torch.empty(st.n, st.d, dtype=torch.float32, device=dev)
        h_cx = torch.empty(2, st.n, dtype=torch.float32, device=dev)
        h_dots = torch.empty(2, dtype=torch.float32, device=dev)
        _lib.check(lib.effdet_episode_supp_loss_backward2(_stream(dev), *st.args(1 if st.thresh_grad else 0),
                                                          ctx.gup.data_ptr(), *(ptr for _, ptr in keep), st.ws.data_ptr(), st.ws_floats,
                                                          d_g.data_ptr(), h_e.data_ptr(), h_cx[0].data_ptr(), h_cx[1].data_ptr(),
                                                          h_dots.data_ptr()), 'effdet_episode_supp_loss_backward2')
        g_shape, e_shape, c_shape, x_shape, m_shape, a_shape = ctx.shapes
        need = ctx.needs_input_grad
        return (d_g.reshape(g_shape) if need[0] else None, h_e.reshape(e_shape), h_cx[0].reshape(c_shape) if st.thresh_grad else None,
                h_cx[1].reshape(x_shape), h_dots[0].reshape(m_shape) if m_shape is not None and need[4] and st.thresh_grad else None,
                h_dots[1].reshape(a_shape) if a_shape is not None and need[5] and st.thresh_grad else None, None)


def support_loss(proj_embds, confs, cls_logits, sel, dot_mult, dot_add, sim_target='max', thresh_grad=True):
    """infer.py:645-658: the meta phase's inner loss, `F.binary_cross_entropy_with_logits(cls_logits, target)` on the target of
    :648 / :652, from the decisions `cluster` took, on the HIP kernels of csrc/episode_support.hip at every order the meta phase
    needs: the value, `torch.autograd.grad(loss, ..., create_graph=True)` and the backward through that gradient.  proj_embds [n, d]
    un-normalised ProjectionNet outputs, confs [n] the confidence logits, cls_logits [n] the class logits (the same tensor as
    confs without FLAGS.separate_head; autograd adds the two gradients), dot_mult / dot_add numbers or tensors.  `sel` is the dict
    `cluster` returns; only proto0, valid, proto (and nearest for 'max') are read, and indices outside their range are clamped
    into it by the kernels.  thresh_grad=False is FLAGS.inner_thresh_train off (infer.py:611): soft_thresh is a constant at
    every order and confs / dot_mult / dot_add get no gradient through it.  The target is not confined to [0, 1]; the formula
    max(x, 0) - x t + log1p(exp(-|x|)) holds as it is.  Returns dict(loss: 0-d, target: [n] detached, equal to cluster's).
    An empty valid set gives NaN loss, target and gradients for 'max', as the reference does.  Third order is not built.  With
    nothing requiring grad only the forward runs; without create_graph the gradient records nothing."""
    use_max = _use_max(sim_target)
    _check(proj_embds, 2, 'support_loss')
    n = proj_embds.shape[0]
    dev = proj_embds.device
    _check_vector(confs, dev, torch.float32, n, 'support_loss', 'confs')
    _check_vector(cls_logits, dev, torch.float32, n, 'support_loss', 'cls_logits')
    m, idx = _sel_indices(sel, dev, n, use_max, 'support_loss')
    loss, target = _SupportLoss.apply(proj_embds, confs, cls_logits, dot_mult, dot_add, idx, m, use_max, bool(thresh_grad))
    return {'loss': loss, 'target': target}


def plan_inner_update(names, n_lr, only_final=False, separate_head=False):
    """Which step size updates which `class_net` parameter, by the rule of infer.py:663-671 on the parameter's name: for every
    name the index into `learnable_lr` (0 <= index < n_lr), or None for a parameter that passes through unchanged.  Pure host
    code.  Pass through: 'bn_' in the name; only_final and 'predict_p' not in it; separate_head and 'predict_p' in it without
    'sep'.  Otherwise 'predict_dw' takes learnable_lr[-2], 'predict_p' takes learnable_lr[-1] and everything else
    learnable_lr[int(name[7])] (the layer digit of 'conv_dw0', 'conv_pw1', ...).  Python's negative indexing is part of the
    rule - with only_final the script builds ONE step size and [-1] finds it - so the result is the index the script's
    expression selects, normalised to [0, n_lr).  ValueError (naming the parameter) where the script's expression would raise
    IndexError or ValueError: a list too short for the name, or a name without a digit at position 7."""
    n_lr = int(n_lr)
    if n_lr < 1:
        raise ValueError('plan_inner_update: at least one step size is needed')
    plan = []
    for n in names:
        if 'bn_' in n or (only_final and 'predict_p' not in n) or (separate_head and 'predict_p' in n and 'sep' not in n):
            plan.append(None)
            continue
        if 'predict_dw' in n:
            k = -2
        elif 'predict_p' in n:
            k = -1
        else:
            try:
                k = int(n[7])
            except (IndexError, ValueError):
                raise ValueError('plan_inner_update: parameter %r has no layer digit at position 7 (infer.py:671)' % (n,)) from None
        if not -n_lr <= k < n_lr:
            raise ValueError('plan_inner_update: parameter %r selects learnable_lr[%d], but there are only %d step sizes' % (n, k, n_lr))
        plan.append(k % n_lr)
    return plan


def _inner_update_launches(index, max_tensors):
    """the positions 0 .. len(index) - 1 in runs of at most max_tensors: one launch each"""
    return [range(s, min(s + max_tensors, len(index))) for s in range(0, len(index), max_tensors)]


def _lr_table(lr_spec, lrs):
    """lr_spec[k]: position of step size k among the tensors `lrs`, or its Python value -> the two host arrays of the C ABI"""
    ptr = [lrs[v].data_ptr() if isinstance(v, int) else None for v in lr_spec]
    val = [0.0 if isinstance(v, int) else v[0] for v in lr_spec]
    return _ptrs(ptr), (ctypes.c_float * len(val))(*val)


class _InnerUpdate(torch.autograd.Function):
    """effdet_inner_update over the whole list; effdet_inner_update_backward is its (once-differentiable) backward.  The outer
    loop calls plain .backward() and p - lr g is bilinear, so nothing of higher order is needed: the second-order terms of MAML
    enter through g's own graph, which the cotangent dg reaches."""

    @staticmethod
    def forward(ctx, lr_spec, index, *tensors):
        lib = _lib.load()
        n_l, n = sum(isinstance(v, int) for v in lr_spec), len(index)
        lrs, ps, gs = tensors[:n_l], tensors[n_l:n_l + n], tensors[n_l + n:]
        dev = ps[0].device
        pc = [p.detach().contiguous() for p in ps]
        gc = [g.detach().contiguous() for g in gs]
        outs = [torch.empty(p.shape, dtype=torch.float32, device=dev) for p in pc]
        lr_ptr, lr_val = _lr_table(lr_spec, lrs)
        st = _stream(dev)
        for run in _inner_update_launches(index, lib.effdet_inner_update_max_tensors()):
            _lib.check(lib.effdet_inner_update(st, len(run), _ptrs([pc[t].data_ptr() for t in run]), _ptrs([gc[t].data_ptr() for t in run]),
                                               _ptrs([outs[t].data_ptr() for t in run]), _lls([pc[t].numel() for t in run]),
                                               _ints([index[t] for t in run]), len(lr_spec), lr_ptr, lr_val), 'effdet_inner_update')
        ctx.lr_spec, ctx.index = lr_spec, index
        ctx.lr_shapes = [t.shape for t in lrs]
        ctx.save_for_backward(*lrs, *gc)             # detached aliases share the version counters: an in-place change raises
        ctx.set_materialize_grads(False)
        return tuple(outs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grad_outs):
        lib = _lib.load()
        lr_spec, index = ctx.lr_spec, ctx.index
        n_l, n = len(ctx.lr_shapes), len(index)
        saved = ctx.saved_tensors
        lrs, gc = saved[:n_l], saved[n_l:]
        need = ctx.needs_input_grad[2:]
        need_lr, need_p, need_g = need[:n_l], need[n_l:n_l + n], need[n_l + n:]
        live = [t for t in range(n) if grad_outs[t] is not None]
        d_lr, d_g = [None] * n_l, [None] * n
        want_lr = any(need_lr)
        if live and (want_lr or any(need_g[t] for t in live)):
            dev = gc[0].device
            G = {t: grad_outs[t].detach().to(dtype=torch.float32).contiguous() for t in live}
            for t in live:
                if need_g[t]:
                    d_g[t] = torch.empty(gc[t].shape, dtype=torch.float32, device=dev)
            lr_ptr, lr_val = _lr_table(lr_spec, lrs)
            runs = [[live[i] for i in r] for r in _inner_update_launches(live, lib.effdet_inner_update_max_tensors())]
            ws = ws_doubles = dlr = None
            if want_lr:
                ws_doubles = max(lib.effdet_inner_update_workspace_doubles(len(r), _lls([gc[t].numel() for t in r])) for r in runs)
                ws = torch.empty(ws_doubles, dtype=torch.float64, device=dev)
                dlr = torch.empty(len(lr_spec), dtype=torch.float32, device=dev)
            st = _stream(dev)
            for i, r in enumerate(runs):            # one stream: a later run reuses the partials' space after the earlier one has added them up
                _lib.check(lib.effdet_inner_update_backward(
                    st, len(r), _ptrs([G[t].data_ptr() for t in r]), _ptrs([gc[t].data_ptr() for t in r]),
                    _ptrs([d_g[t].data_ptr() if d_g[t] is not None else None for t in r]), _lls([gc[t].numel() for t in r]),
                    _ints([index[t] for t in r]), len(lr_spec), lr_ptr, lr_val, ws.data_ptr() if want_lr else None,
                    ws_doubles if want_lr else 0, 1 if i > 0 else 0, dlr.data_ptr() if want_lr else None), 'effdet_inner_update_backward')
            if want_lr:
                used = {index[t] for t in live}
                for k, v in enumerate(lr_spec):
                    if isinstance(v, int) and need_lr[v] and k in used:
                        d_lr[v] = dlr[k].reshape(ctx.lr_shapes[v])
        d_p = [grad_outs[t] if need_p[t] else None for t in range(n)]
        return (None, None, *d_lr, *d_p, *d_g)


def inner_update(named_params, inner_grad, learnable_lr, only_final=False, separate_head=False):
    """infer.py:660-678, the MAML inner update, on the HIP kernels of csrc/inner_update.hip: one launch forward and at most two
    backward for the whole list.  named_params: `class_net.named_parameters()` or any iterable of (name, tensor) - leaves or
    earlier fast weights (the FLAGS.steps > 1 loop); inner_grad: the tuple `torch.autograd.grad(supp_class_loss, params,
    allow_unused=True, create_graph=True)` returned, in the same order; learnable_lr: the step sizes, each a 0-d or 1-element
    float32 GPU tensor (Parameter or not; read on the device when the kernel runs, so nothing synchronises and a captured graph
    sees a value changed in place) or a Python number (travels by value, gets no gradient).  `plan_inner_update` chooses the
    step size of every parameter from its name.  Returns the fast-weight list in the order `MetaHead.forward(fast_weights=...)`
    slices it: par - par_lr * inner_grad with torch's two roundings for an updated parameter, and the SAME object for one that
    passes through.  Deviation from the script: a parameter whose gradient is None (allow_unused) is passed through as the
    same object as well, where `par_lr * None` would raise a TypeError after printing the name.
    Gradients of a later .backward(): to the parameter the cotangent itself, to inner_grad (the entry to the second-order graph)
    -(lr * cotangent), to a step size -sum cotangent * inner_grad over every tensor it updates, accumulated in float64 in a fixed
    order and rounded once (no atomics: two calls give the same bits).  A step size that updates no tensor, or does not require
    grad, gets None, and then no reduction runs.  The backward is once-differentiable.
    Raises for everything unsupported - there is no fallback: CPU or non-float32 tensors, a gradient whose shape differs from
    its parameter's, empty tensors, and a step size tensor on the CPU (infer.py:244-250 creates them there: create them on the
    GPU, `nn.Parameter(torch.tensor(inner_lr, device='cuda'))`).  Non-contiguous tensors are made contiguous."""
    named = list(named_params)
    grads = list(inner_grad)
    lrs_in = list(learnable_lr)
    if len(grads) != len(named):
        raise ValueError('inner_update: %d parameters but %d gradients' % (len(named), len(grads)))
    plan = plan_inner_update([n for n, _ in named], len(lrs_in), only_final, separate_head)
    lib = _lib.load()
    if len(lrs_in) > lib.effdet_inner_update_max_step_sizes():
        raise ValueError('inner_update: at most %d step sizes' % lib.effdet_inner_update_max_step_sizes())
    active = [i for i, k in enumerate(plan) if k is not None and grads[i] is not None]
    dev = None
    for i in active:
        n, p = named[i]
        g = grads[i]
        for what, t in (('parameter', p), ('gradient of', g)):
            if not torch.is_tensor(t) or t.device.type != 'cuda' or t.dtype != torch.float32:
                raise RuntimeError('inner_update: %s %r must be a float32 GPU tensor (no CPU fallback)' % (what, n))
        dev = dev or p.device
        if p.device != dev or g.device != dev:
            raise RuntimeError('inner_update: %r is on another device than the first parameter' % (n,))
        if g.shape != p.shape:
            raise ValueError('inner_update: the gradient of %r has shape %s, the parameter %s' % (n, tuple(g.shape), tuple(p.shape)))
        if p.numel() == 0:
            raise ValueError('inner_update: %r is empty' % (n,))
    lr_spec, lr_tensors = [], []
    for k, v in enumerate(lrs_in):
        if torch.is_tensor(v):
            if v.device.type != 'cuda':
                raise RuntimeError('inner_update: learnable_lr[%d] is on the CPU; create the step sizes on the GPU, '
                                   "e.g. nn.Parameter(torch.tensor(inner_lr, device='cuda')) (no CPU fallback)" % k)
            if v.dtype != torch.float32 or v.numel() != 1 or (dev is not None and v.device != dev):
                raise RuntimeError('inner_update: learnable_lr[%d] must be a 0-d or 1-element float32 tensor on the parameters\' GPU' % k)
            lr_spec.append(len(lr_tensors))
            lr_tensors.append(v)
        else:
            lr_spec.append((float(v),))
    fast = [p for _, p in named]
    if active:
        outs = _InnerUpdate.apply(tuple(lr_spec), tuple(plan[i] for i in active), *lr_tensors, *(named[i][1] for i in active),
                                  *(grads[i] for i in active))
        for i, o in zip(active, outs):
            fast[i] = o
    return fast
