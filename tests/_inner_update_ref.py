"""Reference helpers for episode.plan_inner_update / episode.inner_update: the loop of infer.py:660-678 restated literally, the
MetaHead's parameter names and shapes without a GPU, and seeded tensor lists."""
import numpy as np
import torch


def meta_head_names(layers, levels=5, add_head=False):
    """`MetaHead.named_parameters()` order = the order effdet/meta_head.py registers them in: conv_dw<l>, conv_pw<l>, conv_pb<l> for
    the layers, predict_dw, predict_pw, predict_pb, bn_w<rep><lev> (level-major), bn_b<rep><lev>, and after add_head() predict_pw_sep,
    predict_pb_sep.  It is also the order `MetaHead.forward(fast_weights=...)` slices."""
    names = ['conv_dw%d' % l for l in range(layers)] + ['conv_pw%d' % l for l in range(layers)] + ['conv_pb%d' % l for l in range(layers)]
    names += ['predict_dw', 'predict_pw', 'predict_pb']
    names += ['bn_w%d%d' % (rep, lev) for lev in range(levels) for rep in range(layers)]
    names += ['bn_b%d%d' % (rep, lev) for lev in range(levels) for rep in range(layers)]
    if add_head:
        names += ['predict_pw_sep', 'predict_pb_sep']
    return names


def meta_head_shapes(F, layers, levels=5, anchors=9, add_head=False):
    """(name, shape) of every MetaHead parameter at width F, in named_parameters() order"""
    shape = {'conv_dw': (F, 1, 3, 3), 'conv_pw': (F, F, 1, 1), 'conv_pb': (F,), 'predict_dw': (F, 1, 3, 3), 'predict_pw': (anchors, F, 1, 1),
             'predict_pb': (anchors,), 'bn_': (F,)}
    out = []
    for n in meta_head_names(layers, levels, add_head):
        key = next(k for k in ('predict_dw', 'predict_pw', 'predict_pb', 'conv_dw', 'conv_pw', 'conv_pb', 'bn_') if n.startswith(k))
        out.append((n, shape[key]))
    return out


def literal_update(named_parameters, inner_grad, learnable_lr, only_final=False, separate_head=False, skip_none=False):
    """infer.py:660-678 as the script has it, with FLAGS.only_final / FLAGS.separate_head as arguments.  skip_none: a parameter
    whose gradient is None passes through (the project's documented deviation) instead of raising the script's TypeError."""
    out = []
    for pos, (name, param) in enumerate(named_parameters):
        keep = 'bn_' in name or (only_final and 'predict_p' not in name) or (separate_head and 'predict_p' in name and 'sep' not in name)
        if not keep:
            if 'predict_dw' in name:
                step = learnable_lr[-2]
            elif 'predict_p' in name:
                step = learnable_lr[-1]
            else:
                step = learnable_lr[int(name[7])]
            keep = inner_grad[pos] is None and skip_none
        out.append(param if keep else param - step * inner_grad[pos])
    return out


class _Slot:
    """stands for learnable_lr[k] in literal_update: `par - slot * grad` records k"""

    def __init__(self, k):
        self.k = k

    def __mul__(self, other):
        return self

    def __rsub__(self, other):
        return self


def literal_plan(names, n_lr, only_final=False, separate_head=False):
    """the step-size index the literal loop selects per name (None: the parameter itself comes back); raises what the script raises"""
    pars = [object() for _ in names]
    fast = literal_update(list(zip(names, pars)), [1.0] * len(names), [_Slot(k) for k in range(n_lr)], only_final, separate_head)
    return [None if f is p else f.k for f, p in zip(fast, pars)]


def seeded_list(seed, named_shapes, offset_view=()):
    """-> (params, grads, cotangents): float32 CPU tensors ~ N(0, 1) per (name, shape); a name in offset_view is a view one float
    (4 bytes) into a storage of its own"""
    rs = np.random.RandomState(seed)
    out = ([], [], [])
    for n, shape in named_shapes:
        count = int(np.prod(shape))
        for lst in out:
            if n in offset_view:
                lst.append(torch.from_numpy(rs.standard_normal(count + 1).astype(np.float32))[1:].reshape(shape))
            else:
                lst.append(torch.from_numpy(rs.standard_normal(count).astype(np.float32)).reshape(shape))
    return out


def lr_grad_f64(cotangents, grads, plan, n_lr):
    """d lr_k = -sum_{t: plan[t] = k} sum_i G_t[i] g_t[i] in float64 from the float32 inputs; None for a step size nothing uses"""
    tot = [None] * n_lr
    for G, g, k in zip(cotangents, grads, plan):
        if k is None or g is None or G is None:
            continue
        tot[k] = (tot[k] if tot[k] is not None else 0.0) - float((G.double() * g.double()).sum())
    return tot
