"""Seeded MetaHead cases at every BiFPN width, shared by tests/test_meta_head_widths_host.py (which checks on the CPU that the
inputs are well conditioned and that the statistics yardstick discriminates) and tests/test_meta_head_widths_gpu.py (which runs
the kernels on them).  Nothing here builds a model: the head's weights come from `_seeded.seeded_tensor`, keyed by the
`class_net.*` state-dict names, for the `fpn_channels` / `box_class_repeats` of the width's config.

The yardstick is `oracle.model.meta_head_forward(..., dtype=torch.float64)`.
"""
import numpy as np
import torch

from _seeded import meta_lists, seeded_array, seeded_tensor

# (config, fpn_channels, box_class_repeats): the widths the project supports
WIDTHS = [('tf_efficientdet_d0', 64, 3), ('tf_efficientdet_d1', 88, 3), ('tf_efficientdet_d2', 112, 3),
          ('tf_efficientdet_d3', 160, 4), ('tf_efficientdet_d4', 224, 4), ('tf_efficientdet_d5', 288, 4)]
NAME_OF = {f: n for n, f, _ in WIDTHS}
B = 2
# partial edge tiles in both directions for the 8 x 8 (float32) and 8 x 16 (bf16) tilings, several tiles per level, non-square maps
MAIN_LEVELS = [(12, 20), (20, 12), (5, 3), (2, 2), (1, 2)]
# batch statistics over 4 and 2 samples per channel
FEW_LEVELS = [(4, 4), (1, 2), (1, 1)]
FEW_LEVELS_FALLBACK = [(2, 2), (1, 2)]
GRAD_LEVELS = [(5, 3), (2, 2), (1, 2)]
SEED_BASE, SEED_TRIES = 101, 8

# Seeds accepted by the conditioning checks of tests/test_meta_head_widths_host.py (searched upwards from SEED_BASE, at most
# SEED_TRIES each; that test re-checks every entry).  Main inputs: float32 CPU oracle within a tenth of the float32 bound of
# the float64 oracle and every per-channel batch variance >= 1e-3.  Few-sample inputs: the first condition only; a width
# where none of the 8 seeds passed on FEW_LEVELS has FEW_LEVELS_FALLBACK.
MAIN_SEED = {64: 101, 88: 101, 112: 101, 160: 101, 224: 101, 288: 101}
# (F = 288: seeds 101 and 102 miss the limit of 2e-5, 103 measures 1.7e-5, 104 misses, 105 measures 2.0e-6; 105 is taken so that
# the host check does not sit on its limit.  No width needed the fallback list.)
FEW_CASE = {64: (101, FEW_LEVELS), 88: (102, FEW_LEVELS), 112: (103, FEW_LEVELS), 160: (101, FEW_LEVELS),
            224: (102, FEW_LEVELS), 288: (105, FEW_LEVELS)}

F32_BOUND = 2e-4            # the project's float32 bound: max|a - b| <= 2e-4 * max(1, |b|max)  (test_meta_head_forward)
BF16_RMS_BOUND = 0.05       # and its bf16 bound on the relative rms error


def config_of(name):
    from ood_object_detection_amd.effdet.config import get_efficientdet_config
    return get_efficientdet_config(name)


def head_weights(name, seed, fpn_channels=None):
    """-> (cfg, init, extra): the `class_net.*` state dict a MetaHead is initialised from and its own predict parameters,
    BN affine parameters perturbed as tests/test_model_gpu.py::_meta_head does (1 + 0.2 n, 0.1 n).  `fpn_channels` overrides the
    config's width (the refusal test)."""
    cfg = config_of(name)
    if fpn_channels is not None:
        cfg.fpn_channels = fpn_channels
    Fc, R, L = cfg.fpn_channels, cfg.box_class_repeats, cfg.num_levels
    A = len(cfg.aspect_ratios) * cfg.num_scales
    init = {}
    for r in range(R):
        for k, shape in (('conv_dw.weight', (Fc, 1, 3, 3)), ('conv_pw.weight', (Fc, Fc, 1, 1)), ('conv_pw.bias', (Fc,))):
            k = 'class_net.conv_rep.%d.%s' % (r, k)
            init[k] = seeded_tensor(seed, k, shape)
        for lev in range(L):
            k = 'class_net.bn_rep.%d.%d.bn.' % (r, lev)
            init[k + 'weight'] = torch.from_numpy(1.0 + 0.2 * seeded_array(seed, k + 'weight', (Fc,)))
            init[k + 'bias'] = torch.from_numpy(0.1 * seeded_array(seed, k + 'bias', (Fc,)))
    init['class_net.predict.conv_dw.weight'] = seeded_tensor(seed, 'class_net.predict.conv_dw.weight', (Fc, 1, 3, 3))
    sc = (1.0 / Fc) ** 0.5
    extra = dict(predict_pw=seeded_tensor(seed, 'meta.predict_pw', (A, Fc, 1, 1)) * sc,
                 predict_pb=seeded_tensor(seed, 'meta.predict_pb', (A,)),
                 predict_pw_sep=seeded_tensor(seed, 'meta.predict_pw_sep', (A, Fc, 1, 1)) * sc,
                 predict_pb_sep=seeded_tensor(seed, 'meta.predict_pb_sep', (A,)))
    return cfg, init, extra


def head_lists(cfg, init, extra):
    """the oracle's argument lists: conv_dw, conv_pw, conv_pb, predict, bn_w, bn_b (level-major)"""
    return meta_lists(init, extra, cfg.num_levels, cfg.box_class_repeats)


def build_meta_head(name, seed, sep_head=False):
    """-> (cfg, init, extra, MetaHead on the CPU) without building a model"""
    from ood_object_detection_amd.effdet.meta_head import MetaHead
    cfg, init, extra = head_weights(name, seed)
    mh = MetaHead(cfg, pretrain_init=init)
    if sep_head:
        mh.add_head()
    with torch.no_grad():
        mh.predict_pw.copy_(extra['predict_pw']); mh.predict_pb.copy_(extra['predict_pb'])
        if sep_head:
            mh.predict_pw_sep.copy_(extra['predict_pw_sep']); mh.predict_pb_sep.copy_(extra['predict_pb_sep'])
    return cfg, init, extra, mh


def level_inputs(seed, Fc, levels, batch=B):
    return [torch.from_numpy(seeded_array(seed, 'lvl%d' % i, (batch, Fc, h, w))) for i, (h, w) in enumerate(levels)]


def oracle(cfg, init, extra, x, dtype, **kw):
    from oracle import model as om
    dw, pw, pb, pred, bw, bb = head_lists(cfg, init, extra)
    with torch.no_grad():
        return om.meta_head_forward(dw, pw, pb, bw, bb, pred, x, dtype=dtype, **kw)


def f32_error(a, ref):
    """max|a - ref| / max(1, |ref|max): the quantity the float32 bound is set on"""
    ref = ref.double()
    return float((a.double().cpu() - ref).abs().max()) / max(1.0, float(ref.abs().max()))


def rel_rms(a, ref):
    ref = ref.double()
    return float((a.double().cpu() - ref).norm()) / max(float(ref.norm()), 1e-3)


def min_batch_variance(cfg, init, extra, x):
    """smallest per-channel biased batch variance over every (level, layer), in float64"""
    import torch.nn.functional as F
    dw, pw, pb, pred, bw, bb = head_lists(cfg, init, extra)
    R, low = cfg.box_class_repeats, float('inf')
    D = lambda t: t.double()
    for lev, t in enumerate(x):
        t = D(t)
        for r in range(R):
            t = F.conv2d(F.pad(t, (1, 1, 1, 1)), D(dw[r]), groups=t.shape[1])
            t = F.conv2d(t, D(pw[r]), bias=D(pb[r]))
            low = min(low, float(t.var(dim=(0, 2, 3), unbiased=False).min()))
            t = F.batch_norm(t, None, None, D(bw[lev * R + r]), D(bb[lev * R + r]), training=True, eps=1e-5)
            t = t * torch.sigmoid(t)
    return low


# ---- the layer-level statistics stress grid: one layer, identity convolution, per-channel mean + std * normal
STAT_F = 88
STAT_MEANS, STAT_STDS = (0.0, 1.0, 8.0), (1.0, 0.1, 0.01)
STAT_SHAPES = [(12, 20), (1, 1)]
STAT_SEED = 7
STAT_EPS = 1e-5
# |scale - scale64| <= STAT_BOUND * scale64 and |shift - shift64| <= STAT_BOUND * (|shift64| + 1).  On these exact inputs a
# float32 two-pass computation measures 2.3e-7 at worst and the float32 one-pass formula 1.9e-4 on the least sensitive of the
# cells with mean >= 80 std (n = 480); the bound is their geometric mean, 29 times from either (a first choice of 5e-5 left
# the one-pass side a factor of 4 only).  tests/test_meta_head_widths_host.py re-measures both and asserts a factor of ten.
STAT_BOUND = 6.6e-6


def stat_cell(c):
    """channel -> (mean, std): the nine cells are spread round-robin over the channels"""
    return STAT_MEANS[(c % 9) // 3], STAT_STDS[c % 3]


def stat_input(hw, dtype=torch.float32):
    """[B, STAT_F, H, W] in `dtype` (the values the kernel reads)"""
    h, w = hw
    z = torch.from_numpy(seeded_array(STAT_SEED, 'stat%dx%d' % (h, w), (B, STAT_F, h, w))).double()
    mean = torch.tensor([stat_cell(c)[0] for c in range(STAT_F)], dtype=torch.float64).view(1, -1, 1, 1)
    std = torch.tensor([stat_cell(c)[1] for c in range(STAT_F)], dtype=torch.float64).view(1, -1, 1, 1)
    return (mean + std * z).to(dtype)


def stat_reference(y):
    """scale64 / shift64 of a batch-statistics BN (weight 1, bias 0) from the values `y` [B, C, H, W] themselves"""
    y = y.double()
    var = y.var(dim=(0, 2, 3), unbiased=False)
    scale = 1.0 / torch.sqrt(var + STAT_EPS)
    return scale, -y.mean(dim=(0, 2, 3)) * scale


def stat_errors(scale, shift, y):
    """per channel: |scale - scale64| / scale64 and |shift - shift64| / (|shift64| + 1)"""
    s64, t64 = stat_reference(y)
    return (scale.double().cpu() - s64).abs() / s64, (shift.double().cpu() - t64).abs() / (t64.abs() + 1.0)


def stat_two_pass_f32(y):
    """float32 throughout: mean, then the mean of squared deviations"""
    y = y.float()
    n = y.shape[0] * y.shape[2] * y.shape[3]
    m = y.sum(dim=(0, 2, 3)) / n
    v = ((y - m.view(1, -1, 1, 1)) ** 2).sum(dim=(0, 2, 3)) / n
    sc = 1.0 / torch.sqrt(v + np.float32(STAT_EPS))
    return sc, -m * sc


def stat_one_pass_f32(y, th=8, tw=8):
    """the formula this test was written against: float32 sums of q and q*q per th x tw tile and image, the tiles added in
    double, var = sum(q*q)/n - mean^2"""
    y = y.float()
    Bn, C, H, W = y.shape
    s = torch.zeros(C, dtype=torch.float64); q = torch.zeros(C, dtype=torch.float64)
    for b in range(Bn):
        for y0 in range(0, H, th):
            for x0 in range(0, W, tw):
                t = y[b, :, y0:y0 + th, x0:x0 + tw].reshape(C, -1)
                s += t.sum(1, dtype=torch.float32).double(); q += (t * t).sum(1, dtype=torch.float32).double()
    n = Bn * H * W
    mean = s / n
    var = (q / n - mean * mean).clamp_min(0.0)
    sc = 1.0 / torch.sqrt(var.float() + np.float32(STAT_EPS))
    return sc, -mean.float() * sc


# ---- the differentiable path: autograd through a forward, shared by the float64 reference and the HIP module
def named_leaves(cfg, init, extra, dtype):
    """name (as MetaHead.named_parameters) -> leaf tensor in `dtype`"""
    dw, pw, pb, pred, bw, bb = head_lists(cfg, init, extra)
    R = cfg.box_class_repeats
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_()
    named = {}
    for r in range(R):
        named['conv_dw%d' % r], named['conv_pw%d' % r], named['conv_pb%d' % r] = leaf(dw[r]), leaf(pw[r]), leaf(pb[r])
    named['predict_dw'], named['predict_pw'], named['predict_pb'] = [leaf(t) for t in pred]
    for lev in range(cfg.num_levels):
        for r in range(R):
            named['bn_w%d%d' % (r, lev)], named['bn_b%d%d' % (r, lev)] = leaf(bw[lev * R + r]), leaf(bb[lev * R + r])
    return named


def oracle_from_named(named, cfg, x, dtype):
    from oracle import model as om
    R, L = cfg.box_class_repeats, cfg.num_levels
    return om.meta_head_forward([named['conv_dw%d' % r] for r in range(R)], [named['conv_pw%d' % r] for r in range(R)],
                                [named['conv_pb%d' % r] for r in range(R)],
                                [named['bn_w%d%d' % (r, lev)] for lev in range(L) for r in range(R)],
                                [named['bn_b%d%d' % (r, lev)] for lev in range(L) for r in range(R)],
                                [named['predict_dw'], named['predict_pw'], named['predict_pb']], x, dtype=dtype)


def grad_cotangents(Fc, A, levels, names, shapes):
    """the cotangents / targets / directions of tests/test_model_gpu.py's two gradient tests, at these shapes"""
    go = [seeded_tensor(61, 'go%d' % i, (B, A, h, w)) for i, (h, w) in enumerate(levels)]
    ga = [seeded_tensor(61, 'ga%d' % i, (B, Fc, h, w)) * 0.3 for i, (h, w) in enumerate(levels)]
    go2 = [seeded_tensor(71, 'go%d' % i, (B, A, h, w)) for i, (h, w) in enumerate(levels)]
    vs = [seeded_tensor(72, 'v_' + n, tuple(s)) for n, s in zip(names, shapes)]
    return go, ga, go2, vs


def first_and_second_order(forward, names, params, xs, cot, second=True):
    """forward(xs, ret_activs) -> (outputs, activations) or outputs.  Returns the outputs, d loss / d (params, inputs) for the
    linear loss of test_meta_head_gradients_match_oracle_autograd, and the Hessian-vector product of
    test_meta_head_second_order_matches_oracle_autograd (BCE inner loss), both as name -> tensor or None."""
    go, ga, go2, vs = cot
    to = lambda w, t: w.to(device=t.device, dtype=t.dtype)
    keys = list(names) + ['x%d' % i for i in range(len(xs))]
    outs, acts = forward(xs, True)
    loss = sum((o * to(w, o)).sum() for o, w in zip(outs, go)) + sum((a * to(w, a)).sum() for a, w in zip(acts, ga))
    g = dict(zip(keys, torch.autograd.grad(loss, list(params) + list(xs), allow_unused=True)))
    hv = None
    if second:
        o2 = forward(xs, False)
        inner = sum(torch.nn.functional.binary_cross_entropy_with_logits(o, torch.sigmoid(to(w, o))) for o, w in zip(o2, go2))
        g1 = torch.autograd.grad(inner, list(params), create_graph=True, allow_unused=True)
        assert all(gi is None or gi.requires_grad for gi in g1)
        dot = sum((gi * to(v, gi)).sum() for gi, v in zip(g1, vs) if gi is not None)
        hv = dict(zip(keys, torch.autograd.grad(dot, list(params) + list(xs), allow_unused=True)))
    return [o.detach() for o in outs], [a.detach() for a in acts], g, hv


def oracle_grads(name, seed, levels, dtype):
    """the reference side of the differentiable-path test in `dtype`"""
    cfg, init, extra = head_weights(name, seed)
    named = named_leaves(cfg, init, extra, dtype)
    names = list(named)
    xs = [t.to(dtype).requires_grad_() for t in level_inputs(seed, cfg.fpn_channels, levels)]
    A = len(cfg.aspect_ratios) * cfg.num_scales
    cot = grad_cotangents(cfg.fpn_channels, A, levels, names, [named[n].shape for n in names])

    def fwd(x_, ret_activs):
        o, a = oracle_from_named(named, cfg, x_, dtype)
        return (o, a) if ret_activs else o
    return first_and_second_order(fwd, names, [named[n] for n in names], xs, cot)


def grad_error(got, ref, floor, pb_floor=None):
    """worst over the tensors of max|a - r| / max(|r|max, floor * largest reference gradient), with the tensor's name; a
    gradient the reference does not have must be absent or zero"""
    top = max(float(r.abs().max()) for r in ref.values() if r is not None)
    worst = []
    for n, r in ref.items():
        a = got[n]
        if r is None:
            assert a is None or float(a.abs().max()) == 0.0, n
            continue
        assert a is not None, n
        fl = (pb_floor if (pb_floor is not None and n.startswith('conv_pb')) else floor) * top
        worst.append((float((a.double().cpu() - r.double()).abs().max()) / max(float(r.abs().max()), fl), n))
    worst.sort(reverse=True)
    return worst
