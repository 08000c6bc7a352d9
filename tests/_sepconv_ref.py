"""References of the fused separable conv (csrc/sepconv.hip) for tests/test_sepconv_forms_{host,gpu}.py and the accurate-mode
kernel tests.  No GPU code here.

R64  sep_ref(...): float64 arithmetic of one node / head level - combine -> SiLU -> depthwise 3x3 -> pointwise -> affine -> (SiLU) -
     on inputs and weights that are already rounded to the storage type, in both max-pool pad conventions.
Rq   sep_ref(..., quant=True): the same float64 arithmetic with a bf16 round-to-nearest-even wherever the bf16 kernel stores
     bf16 (read from sepconv_kernel): the fused and activated halo value (store8<T> into the halo tile), the depthwise taps (the
     8x16 tile runs them on the matrix cores as bf16 operands), the depthwise output in the A tile (row_store4<T>), and the output
     unless the call writes float32 (dtype 3).
Defective references (sep_ref(..., defect=...)) are R64 with one fault a kernel could have; the host test shows that the GPU
test's bound separates each of them from R64."""
import torch
import torch.nn.functional as F

from oracle import model as om

DEFECTS = ('shifted last column', 'last 8 channels left out', "other convention's pad_l", 'one tap zeroed')


def bf16_round(x):
    """float64 -> nearest bf16 (ties to even, through float32 as the kernel's float32 values go) -> float64"""
    return x.float().bfloat16().double()


def silu64(y):
    return y * torch.sigmoid(y)


def pool_pads(size, sym):
    """pad before a 3x3 / s2 max pool: TF-SAME (total // 2) or the symmetric convention ('' pad_type: 1)"""
    return 1 if sym else om.same_pad_amounts(size, 3, 2)[0]


def _maxpool(x, pad_t, pad_l):
    """3x3 / s2 max pool of x read with the given pads before; out-of-map taps are -inf; output ceil(size / 2)"""
    H, W = x.shape[-2:]
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    pb, pr = max((Ho - 1) * 2 + 3 - H - pad_t, 0), max((Wo - 1) * 2 + 3 - W - pad_l, 0)
    y = F.max_pool2d(F.pad(x, [pad_l, pr, pad_t, pb], value=float('-inf')), 3, 2, 0)
    return y[..., :Ho, :Wo]


def sep_ref(ins, modes, fw, den, fuse_mode, pre_act, dw, pw, bias, scale, shift, post_act, pool_pad='same', quant=False,
            out_round=True, defect=None):
    """float64 arithmetic of one fused node: combine -> act -> dw3x3 -> pw -> affine -> act.  ins: NCHW maps, modes 0 same size /
    1 nearest x2 / 2 3x3 s2 max pool (pool_pad 'same' or ''); dw [F,1,3,3]; pw [N,F,1,1] (or [N,F]); scale may be None.
    quant: round to bf16 where the bf16 kernel does (out_round False: float32 outputs).  defect: one of DEFECTS, or None."""
    sym = pool_pad != 'same'
    xs = []
    for x, m in zip(ins, modes):
        x = x.double()
        if m == 1:
            x = F.interpolate(x, scale_factor=2.0, mode='nearest')
        elif m == 2:
            if defect == DEFECTS[2]:
                x = _maxpool(x, pool_pads(x.shape[-2], sym), pool_pads(x.shape[-1], not sym))
            else:
                x = om.maxpool_pad(x, 3, 2, pool_pad)
        xs.append(x)
    if fuse_mode == 0:
        y = xs[0]
    elif fuse_mode == 1:
        y = sum((x * w) / den for x, w in zip(xs, fw))
    else:
        y = sum(x * w for x, w in zip(xs, fw))
    if pre_act:
        y = silu64(y)
    dw = dw.double()
    if quant:
        y, dw = bf16_round(y), bf16_round(dw)
    if defect == DEFECTS[3]:
        dw = dw.clone()
        # a tap of median magnitude: a typical one, neither the largest (easy to see) nor one near zero (which no bound on the
        # output can see: zeroing a tap w changes the output by about |w| |x| |pw|)
        c, t = divmod(int(dw.abs().reshape(-1).argsort()[dw.numel() // 2]), 9)
        dw.view(-1, 9)[c, t] = 0.0
    d = om.conv2d_pad(y, dw, None, 1, 'same', groups=y.shape[1])
    if defect == DEFECTS[0]:
        moved = om.conv2d_pad(F.pad(y, [1, 0, 0, 0])[..., :-1], dw, None, 1, 'same', groups=y.shape[1])
        d = torch.cat([d[..., :-1], moved[..., -1:]], -1)
    if quant:
        d = bf16_round(d)
    pw = pw.double().reshape(pw.shape[0], -1, 1, 1)
    if defect == DEFECTS[1]:
        pw = pw.clone()
        pw[:, -8:] = 0.0
    y = F.conv2d(d, pw, None if bias is None else bias.double())
    if scale is not None:
        y = y * scale.double()[None, :, None, None]
    y = y + shift.double()[None, :, None, None]
    if post_act:
        y = silu64(y)
    return bf16_round(y) if quant and out_round else y


def oracle_f32(ins, modes, fw, den, fuse_mode, pre_act, dw, pw, scale, shift, post_act, pool_pad):
    """the same node through oracle.model's float32 functions (_resample's pool / upsample, _combine, _sepconv)"""
    xs = []
    for x, m in zip(ins, modes):
        x = x.float()
        if m == 1:
            x = F.interpolate(x, scale_factor=2.0, mode='nearest')
        elif m == 2:
            x = om.maxpool_pad(x, 3, 2, pool_pad)
        xs.append(x)
    if fuse_mode == 0:
        y = xs[0]
    elif fuse_mode == 1:                                              # 'fastattn': relu(w), den = sum + 1e-4
        w = torch.tensor(fw, dtype=torch.float32)
        assert abs(float(w.sum() + 0.0001) - den) < 1e-6
        y = om._combine(xs, w, 'fastattn')
    else:
        y = torch.stack(xs, dim=-1).mul(torch.tensor(fw, dtype=torch.float32)).sum(dim=-1)     # 'attn' after its softmax / 'sum'
    if pre_act:
        y = om.silu(y)
    sd = {'c.conv_dw.weight': dw.float(), 'c.conv_pw.weight': pw.float().reshape(pw.shape[0], -1, 1, 1)}
    y = om._sepconv(y, sd, 'c.', 'same')
    if scale is not None:
        y = y * scale.float()[None, :, None, None]
    y = y + shift.float()[None, :, None, None]
    return om.silu(y) if post_act else y


def ood_ref(logits):
    """[..., C] float64 logits -> (energy = -logsumexp, max logit)"""
    return -torch.logsumexp(logits, dim=-1), logits.max(dim=-1).values


def energy_carry(logits, BN, rescale=True):
    """energy as the kernel carries it over an anchor's sub-chunks of BN classes: running max m and sum-exp s, s rescaled by
    exp(m - new max) when a later sub-chunk raises the max.  rescale=False is the defective carry that forgets to."""
    C = logits.shape[-1]
    m = torch.full(logits.shape[:-1], float('-inf'), dtype=torch.float64)
    s = torch.zeros(logits.shape[:-1], dtype=torch.float64)
    for c0 in range(0, C, BN):
        z = logits[..., c0:c0 + BN]
        mc = z.max(dim=-1).values
        sc = torch.exp(z - mc[..., None]).sum(dim=-1)
        nm = torch.maximum(m, mc)
        keep = torch.exp(m - nm) if rescale else torch.ones_like(s)
        s = s * keep + sc * torch.exp(mc - nm)
        m = nm
    return -(m + torch.log(s))
