"""float64 reference, seeded inputs and yardsticks of the fused MBConv front half, shared by tests/test_mbconv_variants_host.py
(CPU) and tests/test_mbconv_variants_gpu.py.  No GPU code.

    expand 1x1 (x [* gate]) -> BN1 -> SiLU -> depthwise k x k (stride 1|2, TF-SAME or symmetric padding) -> BN2 -> SiLU

Yardsticks (per output element, `bound()`):
    float32         TOL[float32] = 2e-5 of max|ref|             (tests/test_kernels_gpu.py)
    two-term bf16   TOLP = 4e-5 of max|ref|                     (tests/test_accurate_gpu.py)
    bf16            1.1 u (3 amp + [roll, wide] 1.1 ampz) + half_ulp_bf16(ref) + 1e-5,  u = 2^-8,
                    amp = |s2| sum_taps |w| |e|,  ampz = |s2| sum_taps |w| z  with  z = |s1| sum_c |w1_c| |x_c [g_c]|.

The bf16 bound is derived from the roundings the bf16 kernels make, in the standard model fl(v) = v (1 + d), |d| <= u, where u =
2^-8 is bfloat16's unit roundoff (8 significand bits, round to nearest); SiLU's slope is at most 1.1; float32 accumulation and
the hardware exp / rcp sit in the 1e-5.  It starts from the bound test_kernels_gpu._check_pool_against_oracle derives for the
POOLED value, 2^-9 (2 * 1.1 amp + |ref|) + 1e-5, which charges 2^-9 |e| for holding the expanded map as bf16, the same again
for the bf16 fold of BN1's scale into the expand weights, and 2^-9 |ref| for the output's rounding.  Averaged over a map that
holds; element by element it does not, and the MI355X run of these tests showed it (deep / front up to 1.10, roll / wide 1.2 -
3.7 times that bound with errors scattered over the map, pool sums inside theirs):
  * 2^-9 is the relative half-ulp at the TOP of a binade only; at the bottom it is 2^-8.  The float64 reference itself, correctly
    rounded to bf16, breaks 2^-9 |ref| wherever BN2's shift dominates the taps (test_bf16_element_bound_needs_the_half_ulp).  The
    output's rounding is therefore charged its exact half-ulp, 2^(floor(log2 |ref|) - 8), and the intermediate roundings u.
  * the expanded map: the reference rounds its e to bf16 and the kernel its own; each lies within u |e| of the unrounded value,
    so the two differ by up to 2 u |e| per element (a rounding that falls the other way is a whole ulp): 1.1 * 2 u amp.
  * the taps: every bf16 form runs the depthwise taps on the matrix cores and rounds each tap to bf16 for it (roll / wide with
    BN2's scale folded in): u |w| per tap, 1.1 u amp.  The pooled derivation has no such term.
  * roll / wide fold BN1's scale (and a gate) into the bf16 expand weights: each product w1 s1 [g] is rounded, u |w1 s1 g| |x|
    per term of the dot product - an error relative to sum |w1| |x| (z above), not to |e|, which cancellation makes several
    times smaller.  It passes SiLU (1.1) and the taps: 1.1 * 1.1 u ampz.  deep / front apply BN1 in float32: no such term.
    (The reference multiplies a gate in exactly for these forms; the float32 / spatial forms round x * g to the dtype.)"""
import torch
import torch.nn.functional as F

from oracle import model as om

TOL_F32 = 2e-5            # test_kernels_gpu.TOL[torch.float32]
TOLP = 4e-5               # test_accurate_gpu.TOLP
U_BF16 = 2.0 ** -8        # unit roundoff of bfloat16
TORCH_DTYPE = {0: torch.float32, 1: torch.bfloat16}


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def quantize(t, dtype):
    """the value the storage format of `dtype` holds for t (float32 in, float32 out); the last dimension is the channel dimension"""
    if dtype == 0:
        return t.float()
    if dtype == 1:
        return t.float().to(torch.bfloat16).float()
    from ood_object_detection_amd import pairfmt
    return pairfmt.decode(pairfmt.encode(t.float()))


def make_inputs(case, B, seed=50):
    """seeded operands of a case, as the existing kernel-level tests draw them; x (NHWC) and w1 hold representable values"""
    dtype, gated, Cin, mid, H, W, k, s = case[:8]
    d = dict(B=B)
    d['x'] = quantize(_rand(B, H, W, Cin, seed=seed), dtype)                                   # NHWC
    d['gate'] = torch.sigmoid(_rand(B, Cin, seed=seed + 25)) if gated else None
    d['w1'] = quantize(_rand(mid, Cin, seed=seed + 1, scale=1.5 * Cin ** -0.5), dtype)
    g = torch.Generator().manual_seed(seed + 5)
    d['s1'], d['t1'] = torch.rand(mid, generator=g) + 0.5, _rand(mid, seed=seed + 2, scale=0.2)
    d['wd'] = _rand(mid, 1, k, k, seed=seed + 3, scale=1.0 / k)
    d['s2'], d['t2'] = torch.rand(mid, generator=g) + 0.5, _rand(mid, seed=seed + 4, scale=0.2)
    return d


def _silu(z):
    return z * torch.sigmoid(z)


def folds(case):
    """does the kernel of this case fold BN1's scale (and a gate) into bf16 expand weights?  (bf16 roll / wide)"""
    return case[0] == 1 and case[8][2] in (1, 2)


def expanded(case, d):
    """float64 expanded map [B, mid, H, W] as the kernel of this dtype holds it (bf16: rounded to bf16; the gated input of the
    float32 / bf16 spatial form is rounded to the dtype; the rolling-window forms fold the gate into the weights and the two-term
    form multiplies the value in float32 precision or better: exact product)"""
    dtype = case[0]
    x = d['x'].double()
    if d['gate'] is not None:
        x = x * d['gate'].double()[:, None, None, :]
        if dtype != 2 and not folds(case):
            x = quantize(x.float(), dtype).double()
    z = (x @ d['w1'].double().t()) * d['s1'].double() + d['t1'].double()
    e = _silu(z).permute(0, 3, 1, 2).contiguous()
    if dtype == 1:
        e = e.float().to(torch.bfloat16).double()
    return e


def _dw(e, wd, s, pad):
    return om.conv2d_pad(e, wd, None, s, pad, groups=wd.shape[0])


def reference(case, d, pad='same', e=None):
    """-> (ref, amp, e): float64 output [B, mid, Ho, Wo], the amplitudes behind it (see bound(): amp, or (amp, ampz) for the
    forms that fold BN1's scale into bf16 weights), the expanded map"""
    k, s = case[6], case[7]
    e = expanded(case, d) if e is None else e
    wd, s2, t2 = d['wd'].double(), d['s2'].double()[None, :, None, None], d['t2'].double()[None, :, None, None]
    ref = _silu(_dw(e, wd, s, pad) * s2 + t2)
    amp = _dw(e.abs(), wd.abs(), s, pad) * s2.abs()
    if folds(case):
        x = d['x'].double().abs()
        if d['gate'] is not None:
            x = x * d['gate'].double()[:, None, None, :]
        z = ((x @ d['w1'].double().abs().t()) * d['s1'].double().abs()).permute(0, 3, 1, 2).contiguous()
        amp = (amp, _dw(z, wd.abs(), s, pad) * s2.abs())
    return ref, amp, e


def wrong_reference(case, d, ref, e, pad='same'):
    """the reference with the depthwise window of the LAST output column shifted by one input pixel to the right: what a kernel
    computes that confuses the two padding conventions, or mis-places the last (ragged) strip"""
    k, s = case[6], case[7]
    shifted = F.pad(e[..., 1:], [0, 1])
    wd, s2, t2 = d['wd'].double(), d['s2'].double()[None, :, None, None], d['t2'].double()[None, :, None, None]
    out = ref.clone()
    out[..., -1] = _silu(_dw(shifted, wd, s, pad) * s2 + t2)[..., -1]
    return out


def bound(case, ref, amp):
    """per-element yardstick (see the module docstring)"""
    dtype = case[0]
    if dtype == 0:
        return torch.full_like(ref, TOL_F32 * float(ref.abs().max()))
    if dtype == 2:
        return torch.full_like(ref, TOLP * float(ref.abs().max()))
    amp, ampz = amp if isinstance(amp, tuple) else (amp, None)
    b = 1.1 * U_BF16 * 3 * amp + half_ulp_bf16(ref) + 1e-5
    return b if ampz is None else b + 1.1 * 1.1 * U_BF16 * ampz


def half_ulp_bf16(v):
    """largest error of rounding v to bfloat16 (8 significand bits): 2^(floor(log2 |v|) - 8); 0 for 0"""
    m, ex = torch.frexp(v.abs())                            # |v| = m * 2^ex, 0.5 <= m < 1
    return torch.where(v == 0, torch.zeros_like(v), torch.ldexp(torch.ones_like(v), ex - 9))


def pool_ok(case, pooled, ref, amp):
    """-> worst |pooled - mean(ref)| / bound over (b, c): float32 1e-4 and two-term bf16 2e-5 of max(1, max|mean|) (the project's
    kernel-level tests), bf16 the averaged element bound of test_kernels_gpu._check_pool_against_oracle"""
    dtype = case[0]
    pref = ref.mean((2, 3))
    err = (pooled.double() - pref).abs()
    if dtype == 1:
        amp = amp[0] if isinstance(amp, tuple) else amp
        return float((err / (2.0 ** -9 * (2 * 1.1 * amp + ref.abs()).mean((2, 3)) + 1e-5)).max())
    return float(err.max()) / ((1e-4 if dtype == 0 else 2e-5) * max(1.0, float(pref.abs().max())))


def worst(err, bnd):
    """-> (worst ratio, (b, c, y, x) of it) of an NCHW error against its bound; NaN counts as infinitely wrong"""
    r = torch.nan_to_num(err / bnd, nan=float('inf'))
    i = int(r.argmax())
    idx = []
    for n in reversed(r.shape):
        idx.append(i % n)
        i //= n
    return float(r.max()), tuple(reversed(idx))
