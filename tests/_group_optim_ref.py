"""Reference driver and shared case data of the grouped-optimizer tests (test_group_optim_host.py, test_group_optim_gpu.py).

The yardstick is torch itself: K steps of `torch.optim.Adam` / `torch.optim.SGD` (single-tensor path) and one
`torch.nn.utils.clip_grad_norm_` per clip domain, on the CPU, over a parameter list with given per-step gradients (None where a
parameter received none), with learning-rate edits between steps - in float32 and in float64 on identical values.
`e32(optim)` is the tolerance yardstick: the largest deviation of the float32 run from the float64 run on the six-step scenario,
per quantity (parameters, each state buffer)."""
import functools

import numpy as np
import torch

SHAPES = [(), (3,), (15,), (16,), (17,), (63,), (64,), (65,), (255,), (257,), (8, 3, 3, 3), (64, 40), (4099,), (100003,)]
NORM_ONLY = 7                    # in clip domain 0 and in no group
NEVER = 9                        # receives no gradient in any step
ABSENT = {1: [3], 2: [4]}        # step (1-based) -> tensors without a gradient in that step only
LR_EDIT_STEP, LR_EDIT_GROUP, LR_EDIT_VALUE = 4, 1, 5e-3
STEPS = 6
ACCUMULATED = (5, 6)             # steps whose gradient is the sum of two in-place adds into p.grad
HYPER = {'adam': dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8), 'sgd': dict(lr=1e-2, momentum=0.9, nesterov=True)}


def scenario_groups():
    """group of tensor i = i % 3 (not contiguous in parameter order); NORM_ONLY in none.  Group 1 starts at lr 0, group 2 has weight decay."""
    idx = [[i for i in range(len(SHAPES)) if i % 3 == g and i != NORM_ONLY] for g in range(3)]
    return [{'params': idx[0]}, {'params': idx[1], 'lr': 0.0}, {'params': idx[2], 'weight_decay': 0.1}]


def scenario_domains():
    """two clip domains cut differently from the groups; group 2 is in neither"""
    in_dom = [i for i in range(len(SHAPES)) if i % 3 != 2 or i == NORM_ONLY]
    return [{'params': [i for i in in_dom if i <= NORM_ONLY], 'max_norm': 1.0}, {'params': [i for i in in_dom if i > NORM_ONLY], 'max_norm': 5.0}]


@functools.lru_cache(maxsize=None)
def scenario_data():
    """-> (initial parameters [float32 arrays], grads: per step a list of (a, b) float32 array pairs or None; b is None unless the
    step accumulates two adds).  Small gradients, except in step 2 those of domain 1: exactly that domain clips there."""
    rs = np.random.RandomState(1234)
    p0 = [rs.normal(0, 1, s).astype(np.float32) for s in SHAPES]
    big = set(scenario_domains()[1]['params'])
    grads = []
    for step in range(1, STEPS + 1):
        row = []
        for i, s in enumerate(SHAPES):
            if i == NEVER or i in ABSENT.get(step, []):
                row.append(None)
                continue
            scale = 1.0 if (step == 2 and i in big) else 1e-2
            a = (rs.normal(0, 1, s) * scale).astype(np.float32)
            b = (rs.normal(0, 1, s) * scale).astype(np.float32) if step in ACCUMULATED else None
            row.append((a, b))
        grads.append(row)
    return p0, grads


def summed(pair):
    """the gradient a step sees: a, or a + b added in float32 (what two in-place adds into a zeroed float32 `.grad` leave)"""
    a, b = pair
    return a if b is None else (a + b).astype(np.float32)


def run_reference(optim, p0, grads, groups, domains, dtype, lr_edits=None, hyper=None, steps_before=None):
    """K steps of torch on the CPU.  p0: arrays; grads[k][i]: array or None; groups / domains: dicts whose 'params' are index lists
    (other keys pass through to torch / `max_norm`); lr_edits: {step (1-based): [(group, lr), ...]} applied before that step.
    -> list over steps of {'params', 'state1', 'state2' (lists of float64 arrays, zeros where torch holds no state), 'steps' (Adam's
    per-parameter count; SGD: 1 once a momentum buffer exists), 'norms', 'coefs' (per domain)}, and the torch optimizer."""
    params = [torch.nn.Parameter(torch.from_numpy(np.asarray(a)).to(dtype).clone()) for a in p0]
    tgroups = []
    for g in groups:
        t = {k: v for k, v in g.items() if k != 'params'}
        t['params'] = [params[i] for i in g['params']]
        tgroups.append(t)
    hyper = dict(HYPER[optim] if hyper is None else hyper)
    opt = (torch.optim.Adam if optim == 'adam' else torch.optim.SGD)(tgroups, foreach=False, **hyper)
    out = []
    for k, row in enumerate(grads):
        for gi, lr in (lr_edits or {}).get(k + 1, []):
            opt.param_groups[gi]['lr'] = lr
        for p, g in zip(params, row):
            p.grad = None if g is None else torch.from_numpy(np.asarray(g)).to(dtype).clone()
        norms, coefs = [], []
        for d in domains:
            n = float(torch.nn.utils.clip_grad_norm_([params[i] for i in d['params']], d['max_norm'], foreach=False))
            norms.append(n)
            coefs.append(min(1.0, d['max_norm'] / (n + 1e-6)))
        opt.step()
        snap = {'params': [p.detach().double().numpy().copy() for p in params], 'state1': [], 'state2': [], 'steps': [], 'norms': norms, 'coefs': coefs}
        for p in params:
            st = opt.state.get(p, {})
            zero = np.zeros(tuple(p.shape))
            if optim == 'adam':
                snap['state1'].append(st['exp_avg'].double().numpy().copy() if st else zero)
                snap['state2'].append(st['exp_avg_sq'].double().numpy().copy() if st else zero)
                snap['steps'].append(int(st['step']) if st else 0)
            else:
                buf = st.get('momentum_buffer')
                snap['state1'].append(buf.double().numpy().copy() if buf is not None else zero)
                snap['state2'].append(zero)
                snap['steps'].append(0 if buf is None else 1)
        out.append(snap)
    return out, opt, params


def scenario_reference(optim, dtype):
    p0, grads = scenario_data()
    rows = [[None if g is None else summed(g) for g in row] for row in grads]
    return run_reference(optim, p0, rows, scenario_groups(), scenario_domains(), dtype,
                         lr_edits={LR_EDIT_STEP: [(LR_EDIT_GROUP, LR_EDIT_VALUE)]})[0]


def deviation(run, ref):
    """largest |run - ref| per quantity over all steps and tensors"""
    return {q: max(float(np.abs(a - b).max()) for s, r in zip(run, ref) for a, b in zip(s[q], r[q])) for q in ('params', 'state1', 'state2')}


@functools.lru_cache(maxsize=None)
def scenario_pair(optim):
    """-> (float64 run, E32) of the six-step scenario"""
    ref = scenario_reference(optim, torch.float64)
    return ref, deviation(scenario_reference(optim, torch.float32), ref)


def e32(optim):
    return scenario_pair(optim)[1]


def bound(e, ref_arrays):
    """4 E32 + 1e-7 max(1, |ref|max)"""
    return 4.0 * e + 1e-7 * max(1.0, max(float(np.abs(a).max()) for a in ref_arrays))
