"""References of the inference 1x1-conv GEMM (csrc/pw_gemm.hip) for tests/test_pw_gemm_forms_{host,gpu}.py.  No GPU code here.

R64  ref(...): the operation stated once, in float64, on inputs that already hold the values of the storage type (float32, bf16
     rounded, or the two-term value hi + lo that pairfmt stores):

         C[m, n] = act((sum_k a[m, k] g[img(m), k] w[n, k]) scale[n] + shift[n]) + residual[m, n]     act: none / SiLU / ReLU

     The gate multiplies unrounded products.  The kernel folds it into W and rounds w g to the storage type: that is the kernel's
     error and the GPU test's bound carries it.
Defective references (ref(..., defect=...)) are R64 with one fault a kernel could have; the host test shows that the GPU test's
bound separates each of them from R64 on every case where the fault can occur."""
import torch

from oracle import model as om

DEFECTS = ('one K-chunk of one tile dropped', 'K tail not zeroed', "the neighbouring image's gate", 'channels c and c ^ 4 swapped',
           'residual missing on the last partial 8-channel group', 'residual indexed with ldc', 'last partial pixel tile from pixel 0',
           'SiLU after the residual')
PIX = 128                                     # pixels of a workgroup's tile


def bf16_round(x):
    """float64 -> nearest bf16 (ties to even, through float32 as the kernel's float32 values go) -> float64"""
    return x.float().bfloat16().double()


def stored(x, dtype):
    """float32 tensor -> the float32 values the storage type holds: itself, bf16-rounded, or the two-term value hi + lo"""
    if dtype == 0:
        return x.float()
    if dtype == 1:
        return x.float().bfloat16().float()
    from ood_object_detection_amd import pairfmt
    return pairfmt.decode(pairfmt.encode(x.float()))


def silu64(y):
    return y * torch.sigmoid(y)


def _act(y, act):
    return silu64(y) if act == 1 else (torch.relu(y) if act == 2 else y)


def applicable(defect, d, p):
    """can this fault change the result of the case with inputs d (make_inputs) and plan p?"""
    K, N, rpi, B = d['a'].shape[1], d['w'].shape[0], d['rpi'], d['a'].shape[0] // d['rpi']
    i = DEFECTS.index(defect)
    if i == 0:
        return True
    if i == 1:
        return K % p['KPC'] != 0
    if i == 2:
        return d['gate'] is not None and B > 1
    if i == 3:
        return N > 4
    if i == 4:
        return d['res'] is not None and N % 8 != 0
    if i == 5:
        return d['res'] is not None and d['ldc'] != N and d['a'].shape[0] > 1
    if i == 6:
        return rpi > PIX and rpi % PIX != 0
    return d['res'] is not None and d['act'] == 1


def ref(d, p=None, defect=None, absolute=False):
    """d: the inputs of make_inputs (values as stored) -> float64 [M, N].  p: the plan (a defect that depends on the tile needs
    it).  absolute: the sum of |a g w| |scale| instead - the derived term of the gated bf16 bound."""
    a, w = d['a'].double(), d['w'].double()
    M, K = a.shape
    N, rpi = w.shape[0], d['rpi']
    B = M // rpi
    i = DEFECTS.index(defect) if defect else -1
    scale = torch.ones(N, dtype=torch.float64) if d['scale'] is None else d['scale'].double()
    shift = d['shift'].double()
    gate = None if d['gate'] is None else d['gate'].double()
    if i == 2:
        gate = gate.roll(1, 0)
    if i == 3:
        sw = torch.arange(N) ^ 4
        sw = torch.where(sw < N, sw, torch.arange(N))
        scale, shift = scale[sw], shift[sw]
        if gate is not None:
            gate = gate[:, torch.arange(K) ^ 4]
    ag = a if gate is None else (a.view(B, rpi, K) * gate[:, None, :]).reshape(M, K)
    if i == 6:                                                        # every image's last, partial tile reads the image's first pixels
        t0 = rpi // PIX * PIX
        ag = ag.view(B, rpi, K).clone()
        ag[:, t0:] = ag[:, :rpi - t0].clone()
        ag = ag.reshape(M, K)
    if absolute:
        return (ag.abs() @ w.abs().t()) * scale.abs()
    acc = ag @ w.t()
    if i == 0:                                                        # image 0, pixel tile 0, channel tile 0: a middle K-chunk is lost
        kpc, bn = p['KPC'], p['BN']
        k0 = (p['kchunks'] // 2) * kpc
        rows, cols = min(PIX, rpi), min(bn, N)
        acc[:rows, :cols] -= ag[:rows, k0:k0 + kpc] @ w[:cols, k0:k0 + kpc].t()
    if i == 1:                                                        # the chunk's tail multiplies the row start by the next W row
        kpc = p['KPC']
        t = kpc - K % kpc
        acc += a[:, :t] @ w.roll(-1, 0)[:, :t].t()
    y = _act(acc * scale + shift, 0 if i == 7 else d['act'])
    if d['res'] is not None:
        res = d['res'].double()
        if i == 4:
            res = res.clone()
            res[:, N // 8 * 8:] = 0.0
        if i == 5:
            idx = (torch.arange(M)[:, None] * d['ldc'] + torch.arange(N)[None, :]) % (M * N)
            res = res.reshape(-1)[idx]
        y = y + res
    return _act(y, d['act']) if i == 7 else y


def oracle_f32(d):
    """the same call through oracle.model's float32 functions: a 1x1 conv2d_pad of the gated map, affine, silu / relu, shortcut"""
    a, w = d['a'].float(), d['w'].float()
    M, K = a.shape
    N, rpi = w.shape[0], d['rpi']
    B = M // rpi
    x = a.view(B, rpi, 1, K).permute(0, 3, 1, 2)
    if d['gate'] is not None:
        x = x * d['gate'].float()[:, :, None, None]
    y = om.conv2d_pad(x, w.view(N, K, 1, 1), None, 1, 'same')
    if d['scale'] is not None:
        y = y * d['scale'].float()[None, :, None, None]
    y = y + d['shift'].float()[None, :, None, None]
    y = om.silu(y) if d['act'] == 1 else (torch.relu(y) if d['act'] == 2 else y)
    y = y.permute(0, 2, 3, 1).reshape(M, N)
    return y if d['res'] is None else y + d['res'].float()
