"""The meta phase's support loss (infer.py:645-658) in torch, at the three orders the meta phase uses it: the literal form
(`_episode_ref.cluster_literal(..., sel=)`'s target, n x n matrices and all, + F.binary_cross_entropy_with_logits) and the lean form
of rows and n x m products.  Both take the discrete decisions as given and work on whatever device / dtype their inputs have; they are
differentiated by torch autograd: `create_graph=True`, then a second `grad` of <V, gradient>."""
import torch
import torch.nn.functional as F

import _episode_loss_ref as lref
import _episode_ref as eref

NAMES = ('embds', 'confs', 'logits', 'dot_mult', 'dot_add')


def loss_literal(proj_embds, confs, logits, sel, dot_mult, dot_add, num, sim_target='max', thresh_grad=True):
    """infer.py:607-656 with the decisions of `sel`.  thresh_grad=False: FLAGS.inner_thresh_train off, soft_thresh detached (:611)."""
    if not thresh_grad:                                     # soft_thresh is formed under no_grad
        confs, dot_mult, dot_add = (t.detach() if torch.is_tensor(t) else t for t in (confs, dot_mult, dot_add))
    target = eref.cluster_literal(proj_embds, confs, dot_mult, dot_add, num, 0.5, sim_target, sel=sel)['target']
    return F.binary_cross_entropy_with_logits(logits, target), target.detach()


def loss_lean(proj_embds, confs, logits, sel, dot_mult, dot_add, sim_target='max', thresh_grad=True):
    """The arithmetic of csrc/episode_support.hip's header, from row quantities."""
    e = F.normalize(proj_embds, p=2)
    # sigmoid spelled out: autograd's own sigmoid (and logsigmoid) derivatives form 1 - s, which is 0 from l = 37 on even in float64;
    # through exp and the reciprocal every order comes out as products, so the saturated cases have a yardstick
    s = 1 / (1 + torch.exp(-(dot_mult * (confs + dot_add))))
    if not thresh_grad:
        s = s.detach()
    valid = sel['valid']
    cmean = e[sel['proto0'][valid]].mean(0)
    P = e[sel['proto']]
    if sim_target == 'max':
        nearest = sel['nearest']
        t = s * (P @ cmean)[nearest] * (e * P[nearest]).sum(1)
    else:
        t = s * (e @ P.mean(0))
    x = logits
    loss = (x.clamp(min=0) - x * t + torch.log1p(torch.exp(-x.abs()))).sum() / x.shape[0]
    return loss, t.detach()


def draw(seed, num, rows, d, sim_target, saturated=False):
    """-> dict(x [n, d], confs [n], logits [n] ~ N(0, 2) (float32, CPU), dm, da, sel: the float64 lean decisions, g: the upstream
    scalar, V: the five N(0, 1) cotangents)"""
    x, sat_confs = eref.clustered_rows(seed, num, rows, d)
    n = num * rows
    gen = torch.Generator().manual_seed(1000 + seed)
    confs, dm, da = torch.randn(n, generator=gen), 1.5, 0.25
    logits = 2. * torch.randn(n, generator=gen)
    sel, lean = lref.decisions(x.double(), confs.double(), dm, da, num, sim_target)
    if saturated:
        confs = torch.where(torch.rand(n, generator=gen) < 0.5, -40., 40.) / dm - da
        logits = torch.where(torch.rand(n, generator=gen) < 0.5, -40., 40.)
    g = float(torch.rand((), generator=gen)) + 0.5
    V = [torch.randn(n, d, generator=gen), torch.randn(n, generator=gen), torch.randn(n, generator=gen),
         torch.randn((), generator=gen), torch.randn((), generator=gen)]
    return dict(x=x, confs=confs, logits=logits, dm=dm, da=da, sel=sel, lean=lean, g=g, V=V, num=num)


def orders(case, form, dtype, sim_target='max', thresh_grad=True, shared_head=False, present=(0, 1, 2, 3, 4), second=True):
    """`form` ('lean' / 'literal') in `dtype` on the CPU -> dict(loss, target, grads [5], d_g, hvp [5]); entries of the lists follow
    NAMES, None where nothing flows.  shared_head: logits is confs (gradients add up, entry 2 is None).  `present`: the cotangents
    that are given."""
    leaves = [case['x'].to(dtype).clone().requires_grad_(), case['confs'].to(dtype).clone().requires_grad_(),
              case['logits'].to(dtype).clone().requires_grad_(), torch.tensor(case['dm'], dtype=dtype, requires_grad=True),
              torch.tensor(case['da'], dtype=dtype, requires_grad=True)]
    g = torch.tensor(case['g'], dtype=dtype, requires_grad=True)
    logits = leaves[1] if shared_head else leaves[2]
    if form == 'lean':
        loss, target = loss_lean(leaves[0], leaves[1], logits, case['sel'], leaves[3], leaves[4], sim_target, thresh_grad)
    else:
        loss, target = loss_literal(leaves[0], leaves[1], logits, case['sel'], leaves[3], leaves[4], case['num'], sim_target, thresh_grad)
    grads = torch.autograd.grad(loss, leaves, grad_outputs=g, create_graph=True, allow_unused=True)
    out = dict(loss=loss.detach(), target=target, grads=[None if t is None else t.detach() for t in grads])
    if second:
        scalar = sum((grads[i] * case['V'][i].to(dtype)).sum() for i in present if grads[i] is not None)
        hv = torch.autograd.grad(scalar, [g] + leaves, allow_unused=True)
        out.update(d_g=hv[0], hvp=list(hv[1:]))
    return out
