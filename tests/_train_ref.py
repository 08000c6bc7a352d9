"""Operands and plain references of the cases of tests/_train_cases.py, on the CPU (tests/test_train_forms_{host,gpu}.py).
Two kinds of operands: exact - seeded integers of magnitude 1 ... 3, with which every linear output is an integer that float32
holds exactly in any summation order, so the kernel must EQUAL the int64 reference - and real (_seeded.seeded_array, as the older
tests), compared with float64 at those tests' yardsticks.  Every reference here is float64 computed from the float32 operands;
on integer operands float64 is exact as well (sums far below 2^53)."""
import numpy as np
import torch
import torch.nn.functional as F

import _train_cases as tc
from _seeded import _rs, seeded_array


def exact_values(seed, key, shape):
    """seeded integers from {-3, -2, -1, 1, 2, 3} (never zero) as float32"""
    v = _rs(seed, key).randint(0, 6, size=tuple(int(s) for s in shape))
    return torch.from_numpy(np.array([-3, -2, -1, 1, 2, 3], dtype=np.float32)[v])


def _fill(mode, seed, key, shape, positive=False):
    if mode == 'exact':
        return exact_values(seed, key, shape)
    if mode == 'three':                                   # every operand at the largest magnitude (abs_sum_max)
        return torch.full(tuple(shape), 3.0)
    a = torch.from_numpy(seeded_array(seed, key, tuple(shape)))
    return a.abs() * 0.5 + 0.25 if positive else a        # (gates and BN scales of the real run: positive, order 1)


def level_rows(lv, ld_rows=None):
    """row m of the level-major packed pyramid (level, image, pixel) -> its row b * P + lq0[level] + pixel in the image-major tensor"""
    B, hw = lv
    P = sum(h * w for h, w in hw)
    idx, q0 = [], 0
    for h, w in hw:
        n = h * w
        idx.append((torch.arange(B)[:, None] * P + q0 + torch.arange(n)[None, :]).reshape(-1))
        q0 += n
    return torch.cat(idx), P


def strided_rows(M, rpi):
    m = torch.arange(M)
    return m // rpi, m % rpi


def place(case, dense, cols):
    """the dense logical rows [M, cols] of the non-dense side of a GEMM case inside its image-major tensor, the rest NaN:
    -> flat float32 tensor of tc.packed_floats(case) elements, and the index of the first element of every row in it"""
    M = case[2]
    pk, lv = (case[7], case[8]) if case[0] == 'nt' else (case[6], case[7])
    n = tc.packed_floats(case)
    if lv is not None:
        rows, P = level_rows(lv)
        start = (rows // P) * pk[1] + (rows % P) * pk[2]
    else:
        img, r = strided_rows(M, pk[0])
        start = img * pk[1] + r * pk[2]
    flat = torch.full((n,), float('nan'))
    if dense is not None:
        idx = (start[:, None] + torch.arange(cols)[None, :]).reshape(-1)
        flat[idx] = dense.reshape(-1)
    return flat, start


def gather(flat, start, cols):
    return flat[(start[:, None] + torch.arange(cols)[None, :]).reshape(-1)].reshape(-1, cols)


# ---- operands ---------------------------------------------------------------------------------------------------
def operands(case, mode, seed=5):
    """{name: float32 CPU tensor} of a case: the logical (dense-row) operands"""
    d = {}
    if case[0] == 'nt':
        _, entry, M, K, N, akind, ckind, pk, lv, ops, rows, align = case[:12]
        d['A'], d['W'] = _fill(mode, seed, 'A', (M, K)), _fill(mode, seed, 'W', (N, K))
        if ops & tc.BIAS:
            d['bias'] = _fill(mode, seed, 'bias', (N,))
        if ops & tc.RES:
            d['R'] = _fill(mode, seed, 'R', (M, N))
        if ops & tc.ACC:
            d['prev'] = _fill(mode, seed, 'prev', (M, N))
        if ops & tc.A_SCALE:
            d['gate'] = _fill(mode, seed, 'gate', ((M + rows - 1) // rows, K), positive=True)
        if ops & tc.MASK:
            d['mask'] = _fill('exact' if mode == 'three' else mode, seed, 'mask', (M, N))
    elif case[0] == 'tn':
        _, entry, M, N, K, ykind, pk, lv, rows, align = case[:10]
        d['dY'], d['X'] = _fill(mode, seed, 'dY', (M, N)), _fill(mode, seed, 'X', (M, K))
        if rows:
            d['gate'] = _fill(mode, seed, 'gate', ((M + rows - 1) // rows, K), positive=True)
    else:
        _, which, B, H, W, C, k, s, pad, flag = case[:10]
        Ho, Wo = tc.same_out(H, s), tc.same_out(W, s)
        d['X'] = _fill(mode, seed, 'X', (B, H, W, C))
        d['taps'] = _fill(mode, seed, 'taps', (k * k, C))
        d['scale'], d['shift'] = _fill(mode, seed, 'scale', (C,), positive=True), _fill(mode, seed, 'shift', (C,))
        d['dY'] = _fill(mode, seed, 'dY', (B, Ho, Wo, C))
        d['Zb'] = _fill('exact' if mode == 'three' else mode, seed, 'Zb', (B, H, W, C))     # pre-activation of the layer below (bwd_dx)
    return d


# ---- references -------------------------------------------------------------------------------------------------
def nt_reference(case, d):
    """C [M, N] float64 (after the epilogue of the entry, before C2)"""
    _, entry, M, K, N, akind, ckind, pk, lv, ops, rows, align = case[:12]
    A = d['A'].double()
    if ops & tc.A_SCALE:
        A = A * d['gate'].double()[torch.arange(M) // rows]
    C = A @ d['W'].double().t()
    for name in ('bias', 'R', 'prev'):
        if name in d:
            C = C + d[name].double()
    if tc.EPI[entry] == 1:
        C = torch.relu(C)
    elif tc.EPI[entry] == 2:
        C = torch.where(d['mask'] > 0, C, torch.zeros_like(C))
    return C


def tn_reference(case, d):
    """(dW [N, K], dsum [N]) float64"""
    _, entry, M, N, K, ykind, pk, lv, rows, align = case[:10]
    X = d['X'].double()
    if rows:
        X = X * d['gate'].double()[torch.arange(M) // rows]
    dY = d['dY'].double()
    return dY.t() @ X, dY.sum(0)


def pad_before(n, k, s, sym):
    """rows / columns of zeros before the map: TF-SAME (half of what the last window needs, rounded down) or symmetric (k // 2)"""
    if sym:
        return k // 2
    return max((tc.same_out(n, s) - 1) * s + k - n, 0) // 2


def _conv(x_nchw, w, k, s, pad, H, W):
    pt, pl = pad_before(H, k, s, pad), pad_before(W, k, s, pad)
    y = F.conv2d(F.pad(x_nchw, [pl, k, pt, k]), w, None, s, 0, 1, w.shape[0])
    return y[:, :, :tc.same_out(H, s), :tc.same_out(W, s)]


def dw_reference(case, d):
    """float64, NHWC: fwd -> Z; bwd_dx -> dX (without the SiLU factor); bwd_dw -> (dtaps [k * k, C], dsum [C])"""
    _, which, B, H, W, C, k, s, pad, flag = case[:10]
    x = d['X'].double().permute(0, 3, 1, 2).requires_grad_()
    w = d['taps'].double().t().reshape(C, 1, k, k).clone().requires_grad_()
    y = _conv(x, w, k, s, pad, H, W)
    if which == 'fwd':
        return (y.detach() * d['scale'].double()[None, :, None, None] + d['shift'].double()[None, :, None, None]).permute(0, 2, 3, 1)
    dy = d['dY'].double().permute(0, 3, 1, 2)
    gx, gw = torch.autograd.grad(y, (x, w), dy)
    if which == 'bwd_dx':
        return gx.permute(0, 2, 3, 1)
    return gw.reshape(C, k * k).t(), dy.sum((0, 2, 3))


def silu64(z):
    z = z.double()
    return z * torch.sigmoid(z)


def silu_grad64(z):
    z = z.double()
    sg = torch.sigmoid(z)
    return sg * (1 + z * (1 - sg))


def abs_sum_max(case):
    """the largest sum of |products| any output of the reference of a case can reach with operands of magnitude <= 3: the
    reference on operands that are all 3"""
    d = operands(case, 'three')
    if case[0] == 'nt':
        d.pop('mask', None)
        entry = case[1]
        c = case[:1] + ('gemm_nt_fused' if tc.EPI[entry] else entry,) + case[2:]
        return float(nt_reference(c, d).abs().max())
    if case[0] == 'tn':
        return float(max(t.abs().max() for t in tn_reference(case, d)))
    r = dw_reference(case, d)
    return float(max(t.abs().max() for t in (r if isinstance(r, tuple) else (r,))))
