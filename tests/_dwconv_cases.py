"""Case tables and float64 references of tests/test_dwconv_forms_{host,gpu}.py: the unfused depthwise path of csrc/dwconv.hip -
effdet_dwconv_bn_act, effdet_se_gate, effdet_maxpool_same - in float32 (dtype 0), bf16 (dtype 1) and two-term bf16 (dtype 2).  No
GPU code here: the geometry of a depthwise call is asked of the host-only query effdet_dwconv_plan_describe, which is answered
by the function the launch itself uses.

A depthwise case is (dtype, C, H, W, k, stride); the tests run it under both pad conventions, with act 1 + pool partial sums and
with act 0 + no pool partial.  Channel counts: 8 (one group: 256 pixels in flight, 2048 per workgroup), 144 (18 groups do not
divide 256: 252 threads), 1152 (one pixel in flight), 3072 (two channel slices, the b5 backbone's widest).  Maps: smaller than a
workgroup's share, a partial last workgroup, H or W of 1, odd and even sizes (the conventions differ where stride 2 meets an
even size).

R64  dw_ref(): act(conv(x) scale + shift) in float64 on inputs that hold the values of the storage type.
Defective references: the other convention's pads, one tap dropped at the border (the last output column never reads the last input
column), a pool sum that misses the last pixel of a workgroup's share."""
import ctypes
import zlib

import torch
import torch.nn.functional as F

import _pw_gemm_ref as pr
from oracle import model as om

PAD = 1 << 24                                 # EFFDET_PAD_SYMMETRIC
PLAN_INTS = 10
FIELDS = ('KS', 'nz', 'CG', 'PT', 'threads', 'ppb', 'blocks', 'pad_t', 'pad_l', 'lds')      # slot order of effdet_dwconv_plan_describe
B = 2
F32_TOL, TOLP = 2e-5, 4e-5                    # tests/test_kernels_gpu.py's float32 and tests/test_accurate_gpu.py's two-term tolerance
DTYPE_NAME = {0: 'f32', 1: 'bf16', 2: 'bf16x2'}
MAPS = ((8, 46, 46), (8, 5, 7), (8, 1, 9), (144, 17, 15), (144, 34, 30), (144, 10, 1), (1152, 5, 8), (3072, 4, 3))
DW_CASES = [(dt, C, H, W, k, s) for dt in (0, 1, 2) for C, H, W in MAPS for k in (3, 5) for s in (1, 2)]
DEFECTS = ("the other convention's pads", 'one tap dropped at the border')
SE_C, SE_NBLK, SE_R = (8, 96, 1152, 3072), (1, 2, 17), (1, 4, 8, 9, 128)
POOL_CASES = [(dt, C, H, W, slack) for dt in (0, 1, 2) for C, H, W, slack in ((64, 5, 7, 0), (64, 9, 9, 24), (8, 1, 5, 8), (136, 6, 4, 0), (64, 20, 20, 16))]


def case_id(c):
    return '%s-c%d-%dx%d-k%ds%d' % ((DTYPE_NAME[c[0]],) + tuple(c[1:]))


def plan(lib, dtype, H, W, C, k, stride, pooled=True, sym=False):
    out = (ctypes.c_int * PLAN_INTS)()
    n = lib.effdet_dwconv_plan_describe(dtype | (PAD if sym else 0), H, W, C, k, stride, int(pooled), out, PLAN_INTS)
    if n < 0:
        return None
    assert n == PLAN_INTS, n
    return dict(zip(FIELDS, out))


def case_plan(lib, case, pooled=True, sym=False):
    dt, C, H, W, k, s = case
    return plan(lib, dt, H, W, C, k, s, pooled, sym)


def _gen(what):
    return torch.Generator().manual_seed(zlib.crc32(repr(what).encode()))


def dw_inputs(case):
    dt, C, H, W, k, s = case
    g = _gen(case)
    x = pr.stored(torch.randn(B, H, W, C, generator=g), dt).permute(0, 3, 1, 2).contiguous()      # NCHW values as stored
    return dict(x=x, w=torch.randn(C, 1, k, k, generator=g) / k, scale=torch.rand(C, generator=g) + 0.5,
                shift=torch.randn(C, generator=g) * 0.3)


def pads(size, k, s, sym):
    return ((s - 1) + (k - 1)) // 2 if sym else om.same_pad_amounts(size, k, s)[0]


def _conv(x, w, k, s, pt, pl):
    H, W = x.shape[-2:]
    Ho, Wo = (H + s - 1) // s, (W + s - 1) // s
    pb, pr_ = max((Ho - 1) * s + k - H - pt, 0), max((Wo - 1) * s + k - W - pl, 0)
    xp = F.pad(x, [pl, pr_, pt, pb])
    y = torch.zeros(x.shape[0], x.shape[1], Ho, Wo, dtype=x.dtype)
    for ky in range(k):                                               # tap by tap (a grouped conv2d of thousands of groups is slow)
        for kx in range(k):
            y += xp[..., ky:ky + s * (Ho - 1) + 1:s, kx:kx + s * (Wo - 1) + 1:s] * w[None, :, 0, ky, kx, None, None]
    return y


def dw_ref(case, d, sym, act, defect=None):
    """float64 [B, Ho, Wo, C]; None when the defect cannot change this case"""
    dt, C, H, W, k, s = case
    x, w = d['x'].double(), d['w'].double()
    pt, pl = pads(H, k, s, sym), pads(W, k, s, sym)
    if defect == DEFECTS[0]:
        if (pt, pl) == (pads(H, k, s, not sym), pads(W, k, s, not sym)):
            return None
        pt, pl = pads(H, k, s, not sym), pads(W, k, s, not sym)
    y = _conv(x, w, k, s, pt, pl)
    if defect == DEFECTS[1]:
        xe = torch.zeros_like(x)                                      # the last output column loses the tap on the last input column
        xe[..., -1] = x[..., -1]
        lost = _conv(xe, w, k, s, pt, pl)
        lost[..., :-1] = 0.0
        if float(lost.abs().max()) == 0.0:
            return None
        y = y - lost
    y = y * d['scale'].double()[None, :, None, None] + d['shift'].double()[None, :, None, None]
    if act:
        y = pr.silu64(y)
    return y.permute(0, 2, 3, 1).contiguous()


def dw_oracle_f32(case, d, sym, act):
    dt, C, H, W, k, s = case
    y = om.conv2d_pad(d['x'].float(), d['w'].float(), None, s, '' if sym else 'same', groups=C)
    y = y * d['scale'][None, :, None, None] + d['shift'][None, :, None, None]
    return (om.silu(y) if act else y).permute(0, 2, 3, 1)


def dw_bound(dtype, r64):
    """(bound on max |got - R64|, e_q): float32 2e-5 max |R64|, two-term 4e-5 max |R64|, bf16 2 e_q max |R64| with e_q the error of
    the bf16-rounded reference, measured from the references alone"""
    top = float(r64.abs().max())
    if dtype == 0:
        return F32_TOL * top, None
    if dtype == 2:
        return TOLP * top, None
    e_q = float((pr.bf16_round(r64) - r64).abs().max()) / top
    return 2.0 * e_q * top, e_q


def pool_blocks(y, ppb, nblk, drop_last=False):
    """y: [B, npix, C] float64 values of the stored output -> [B, nblk, C] sums over each workgroup's pixels (drop_last: the
    defective sum that misses a share's last pixel)"""
    out = torch.zeros(y.shape[0], nblk, y.shape[2], dtype=torch.float64)
    for i in range(nblk):
        part = y[:, i * ppb:(i + 1) * ppb]
        out[:, i] = (part[:, :-1] if drop_last else part).sum(1)
    return out


def pool_bound(dtype, y, ppb, nblk):
    """per (image, workgroup, channel): the kernel adds the float32 values it stores, at most ppb of them in a fixed order:
    (ppb - 1) 2^-24 sum |y|; the two-term dtype adds the float32 value before it is split into 16 significand bits: + 2^-16 sum |y|"""
    return ((ppb - 1) * 2.0 ** -24 + (2.0 ** -16 if dtype == 2 else 0.0)) * pool_blocks(y.abs(), ppb, nblk) + 1e-30


# -------------------------------------------------------------------------------------------------------------------- SE gate
def se_inputs(C, nblk, R):
    g = _gen(('se', C, nblk, R))
    rn = lambda *s: torch.randn(*s, generator=g)
    return dict(partial=rn(B, nblk, C) + 0.3, hw=nblk * 7, W1=rn(R, C) * C ** -0.5, b1=rn(R) * 0.1, W2=rn(C, R) * R ** -0.5, b2=rn(C) * 0.1)


def se_ref(d):
    pooled = d['partial'].double().sum(1) / d['hw']
    return torch.sigmoid(pr.silu64(pooled @ d['W1'].double().t() + d['b1'].double()) @ d['W2'].double().t() + d['b2'].double())


def se_oracle_f32(d):
    """oracle.model._se on a map whose mean is the pooled value: the gate is its output over its input"""
    C, R = d['W2'].shape
    x = (d['partial'].float().sum(1) / d['hw'])[:, :, None, None]
    sd = {'se.conv_reduce.weight': d['W1'].view(R, C, 1, 1), 'se.conv_reduce.bias': d['b1'],
          'se.conv_expand.weight': d['W2'].view(C, R, 1, 1), 'se.conv_expand.bias': d['b2']}
    return (om._se(x, sd, 'se.').double() / x.double())[:, :, 0, 0]


# ------------------------------------------------------------------------------------------------------------------- max pool
def pool_inputs(case):
    dt, C, H, W, slack = case
    return pr.stored(torch.randn(B, H, W, C, generator=_gen(case)) - 2.0, dt)       # mostly negative: a zero pad would show


def pool_ref(x, sym):
    """NHWC stored values -> NHWC 3x3 / s2 max pool, exact"""
    return om.maxpool_pad(x.permute(0, 3, 1, 2), 3, 2, '' if sym else 'same').permute(0, 2, 3, 1).contiguous()
