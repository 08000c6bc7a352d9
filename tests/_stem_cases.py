"""Case tables, float64 references and bounds of tests/test_stem_forms_{host,gpu}.py: the three kernels an image enters the network
through - the fused stem + stage-0 depthwise in its tile form (csrc/stem_dw.hip) and its rolling-window form (csrc/stem_roll.hip),
and the unfused effdet_stem_conv[_u8] (csrc/dwconv.hip).  No GPU code here: form and geometry of a fused call are asked of the
host-only query effdet_stem_dw_plan_describe, which is answered by the functions the launch itself uses.

A fused case is (dtype, in_dtype, C, H, W, B): network dtype 0 float32 | 1 bf16 | 2 two-term bf16, image dtype 0 float32 | 1 bf16 |
2 uint8.  The tests run it under both pad conventions where the entry accepts them.  An unfused case is (out_dtype, in_dtype, Cout,
H, W) at B = 2.  Maps (form for bf16 / two-term, C = 32, TF-SAME):
    16x32   roll, 1 strip of 16, 1 band of 8: the minimum geometry, 3 idle waves        (also at B = 1 and B = 10: two rounds of 8)
    15x60   roll, 1 strip of 30 (full width), pad_t = 1                 17x34   roll, 1 strip of 17 (second pixel tile: one column), band of 9
    82x62   roll, 2 strips (16, 15), bands of 21 and 20 rows            42x182  roll, 4 strips (23, 23, 23, 22)
    122x124 roll, 3 strips x 3 bands, last band 19 rows, 3 workgroups per image, 3 idle waves in the last
    14x32, 16x30  tile: Ho = 7, Wo = 15, just below the rolling form's limits          33x35  tile, 2 x 2 tiles, odd W: scalar patch load
    5x5, 1x9, 9x1 tile, one partial tile, H or W of 1, Wo % 4 != 0
    40x36   tile in float32 and at C != 32, with the two-pixel patch load for bf16 into bf16 (C = 32 in bf16 / two-term: roll, 1 strip of 18, 1 band of 20)
Widths: 32 everywhere; 8, 24, 40, 48, 56, 64 on 33x35, 40x36 and 5x5 (tile form only; 64 in bf16 is past 64 KB of LDS; 40 and 56
leave threads idle in the depthwise phase).

R64  ref(): silu(dwconv(silu(conv(x, w) s1 + t1), taps) s2 + t2) in float64 on inputs that hold the stored values (a uint8 image:
(float32(u8) - 255 mean) / (255 std) in float32, the loader's arithmetic, then widened); the unfused reference is its first half e.

Bounds, per element, from the references alone.  float32 2e-5 max |R64|, two-term 4e-5 max |R64| (the project's TOL and TOLP).
bf16: the worst-case sum, no cancellation assumed, of the roundings the kernel's code makes, with u = 2^-8 (bf16 keeps 8 significant
bits) and SiLU's slope <= 1.1:
    tile form (stem_dw.hip)     the patch is staged in LDS as bf16: one rounding of x for a float32 or uint8 image, none for bf16
                                (`In[i] = from_f<T>(vin[q])`); Wk is bf16 as stored and the MFMA accumulates in float32; e is stored
                                to LDS as bf16 (`E + hp * erow`); the depthwise conv runs in float32 on float32 taps; y is rounded
                                once (`from_f<T>(v)`).
    rolling form (stem_roll.hip) the staged row is bf16 (`commit_rows`): as above; the weights are folded w s1 (-log2 e) and rounded
                                to bf16 (`wf[j][c].v[e]`): one more rounding of every product; the stem ring holds bf16
                                (`row_store4`); the depthwise taps are folded taps s2 (-ln 2) and rounded to bf16 (`abits`); y is
                                rounded once.
    A1 = |s1| conv(|x|, |w|),  n1 = roundings of the stem conv's operands (0 .. 2),  de = 1.1 n1 u A1 + u |e|,
    dz2 = |s2| dwconv(de, |taps|) (+ u |s2| dwconv(|e|, |taps|) in the rolling form),  bound = 1.1 dz2 + u |y| + 2e-5 max |R64|;
    the last term is the float32 floor (float32 accumulation, the hardware exp2 / rcp).
    unfused (dwconv.hip stem_kernel)  a uint8 image is normalised and rounded to bf16 (`to_f<T>(from_f<T>(x))`), float32 and bf16
                                images and the float32 weights enter as they are; e is rounded once at the store:
                                bound = 1.1 n1 u A1 + u |e| + 2e-5 max |e|, n1 = 1 for uint8.
Pool partial rows: the stored output partitioned by the plan (16 x 16 tiles row-major | band * nstrips + strip of band_rows x TWo)
against the float64 sums of what the kernel stored, within _dwconv_cases.pool_bound's float32 summation bound; the rolling form
pools the value before the final rounding: + u sum |stored| in bf16, + 2^-16 sum |stored| in the two-term dtype.

Defective references: the other convention's pads; the depthwise conv padded with the stem map's edge value instead of zero; the
last image column never read; a pool row that misses its last pixel."""
import ctypes
import zlib

import torch
import torch.nn.functional as F

import _pw_gemm_ref as pr
from oracle import model as om

PAD = 1 << 24                                 # EFFDET_PAD_SYMMETRIC
EINVAL = -22
PLAN_INTS = 13
FIELDS = ('roll', 'parts', 'pad_t', 'pad_l', 'Ho', 'Wo', 'nx', 'ny', 'bw', 'bh', 'per_image', 'lds', 'vec_in')   # slot order of effdet_stem_dw_plan_describe
U = 2.0 ** -8
F32_TOL, TOLP = 2e-5, 4e-5                    # tests/test_kernels_gpu.py's float32 and tests/test_accurate_gpu.py's two-term tolerance
SLOPE = 1.1                                   # max |silu'| = 1.0998
ESC, EINV = -1.4426950408889634, -0.6931471805599453
DT_NAME, IN_NAME = {0: 'f32', 1: 'bf16', 2: 'bf16x2'}, {0: 'f32', 1: 'bf16', 2: 'u8'}
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)

ROLL_MAPS = ((16, 32), (15, 60), (17, 34), (82, 62), (42, 182), (122, 124))
TILE_MAPS = ((14, 32), (16, 30), (33, 35), (5, 5), (1, 9), (9, 1), (40, 36))
WIDE_MAPS, WIDE_C = ((33, 35), (40, 36), (5, 5)), (8, 24, 40, 48, 56, 64)
DT_PAIRS = ((0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (2, 2))
# the whole product; what the entry refuses under both conventions leaves the table (refused(), checked against the query on the host)
ALL_FUSED = [(dt, it, C, H, W, B) for dt, it in DT_PAIRS for C, H, W, B in
             [(32, h, w, 2) for h, w in ROLL_MAPS + TILE_MAPS] + [(32, 16, 32, 1), (32, 16, 32, 10)] +
             [(c, h, w, 2) for h, w in WIDE_MAPS for c in WIDE_C]]
UNFUSED_CASES = [(dt, it, C, H, W) for dt, it in DT_PAIRS if (dt, it) != (2, 1) for C in (8, 40, 64) for H, W in ((5, 5), (1, 9), (33, 35), (40, 36))]
DEFECTS = ("the other convention's pads", "the depthwise conv padded with the stem map's edge value", 'the last image column never read')


def refused(case, sym):
    """what effdet_stem_dw_fused[_u8] refuses of the table: the two-term dtype has the rolling form only (C = 32, an even left pad -
    an even W under TF-SAME, never under the symmetric convention - and ceil(W / 2) >= 16, ceil(H / 2) >= 8) and takes no bf16 image"""
    dt, it, C, H, W, B = case
    return dt == 2 and (it == 1 or sym or C != 32 or W % 2 == 1 or (W + 1) // 2 < 16 or (H + 1) // 2 < 8)


FUSED_CASES = [c for c in ALL_FUSED if not (refused(c, False) and refused(c, True))]
# launches the fused entry refuses: (dtype, in_dtype, C, H, W, sym, byte offset of X, why)
REFUSALS = ((1, 0, 12, 16, 32, 0, 0, 'C % 8'), (0, 0, 72, 16, 32, 0, 0, 'C > 64'), (1, 2, 72, 33, 35, 0, 0, 'C > 64'),
            (2, 0, 32, 33, 35, 0, 0, 'two-term, odd W'), (2, 2, 40, 16, 32, 0, 0, 'two-term, C != 32'), (2, 0, 32, 16, 32, 1, 0, 'two-term, the pad flag'),
            (2, 2, 32, 16, 30, 0, 0, 'two-term, Wo < 16'), (2, 0, 32, 14, 32, 0, 0, 'two-term, Ho < 8'), (2, 1, 32, 16, 32, 0, 0, 'bf16 image into two-term'),
            (1, 1, 32, 16, 32, 0, 2, 'rolling form, bf16 image off 4 bytes'), (1, 0, 32, 16, 32, 0, 2, 'rolling form, float32 image off 4 bytes'),
            (2, 0, 32, 16, 32, 0, 2, 'rolling form, float32 image off 4 bytes'), (1, 2, 32, 16, 32, 0, 1, 'rolling form, uint8 image off 2 bytes'),
            (2, 2, 32, 16, 32, 0, 1, 'rolling form, uint8 image off 2 bytes'))


def case_id(c):
    return '%s-from-%s-c%d-%dx%d-b%d' % (DT_NAME[c[0]], IN_NAME[c[1]], c[2], c[3], c[4], c[5])


def unfused_id(c):
    return '%s-from-%s-c%d-%dx%d' % (DT_NAME[c[0]], IN_NAME[c[1]], c[2], c[3], c[4])


def plan(lib, dtype, in_dtype, H, W, C, sym=False):
    """the query's slots by name, or None where the launch would refuse"""
    out = (ctypes.c_int * PLAN_INTS)()
    n = lib.effdet_stem_dw_plan_describe(dtype | (PAD if sym else 0), in_dtype, H, W, C, out, PLAN_INTS)
    if n < 0:
        return None
    assert n == PLAN_INTS, n
    return dict(zip(FIELDS, out))


def case_plan(lib, case, sym=False):
    dt, it, C, H, W, B = case
    return plan(lib, dt, it, H, W, C, sym)


def _gen(what):
    return torch.Generator().manual_seed(zlib.crc32(repr(what).encode()))


def norm_consts():
    """255 mean, 255 std as the float32 values the entry points are handed"""
    return (torch.tensor([255.0 * v for v in MEAN], dtype=torch.float32), torch.tensor([255.0 * v for v in STD], dtype=torch.float32))


def image(g, in_dtype, B, H, W):
    """(what the kernel is handed, the float32 values it holds)"""
    if in_dtype == 2:
        xu = torch.randint(0, 256, (B, 3, H, W), generator=g, dtype=torch.uint8)
        m, s = norm_consts()
        return xu, (xu.float() - m.view(1, 3, 1, 1)) / s.view(1, 3, 1, 1)
    x = torch.randn(B, 3, H, W, generator=g)
    if in_dtype == 1:
        x = x.bfloat16()
    return x, x.float()


def fused_inputs(case):
    """raw: the image as handed over; x: its values (float32); w [C, 3, 3, 3] as the weight dtype stores it (bf16 in bf16, float32
    else); taps [C, 1, 3, 3]; the BN folds"""
    dt, it, C, H, W, B = case
    g = _gen(('stem',) + tuple(case))
    raw, x = image(g, it, B, H, W)
    w = torch.randn(C, 3, 3, 3, generator=g) * 0.25
    return dict(raw=raw, x=x, w=w.bfloat16().float() if dt == 1 else w, s1=torch.rand(C, generator=g) + 0.5, t1=torch.randn(C, generator=g) * 0.2,
                taps=torch.randn(C, 1, 3, 3, generator=g) * 0.35, s2=torch.rand(C, generator=g) + 0.5, t2=torch.randn(C, generator=g) * 0.2)


def unfused_inputs(case):
    dt, it, C, H, W = case
    g = _gen(('stem_conv',) + tuple(case))
    raw, x = image(g, it, 2, H, W)
    return dict(raw=raw, x=x, w=torch.randn(C, 3, 3, 3, generator=g) * 0.25, s1=torch.rand(C, generator=g) + 0.5, t1=torch.randn(C, generator=g) * 0.2)


def pads(size, sym):
    return 1 if sym else om.same_pad_amounts(size, 3, 2)[0]


def _ch(v):
    return v.double()[None, :, None, None]


def stem_conv(x, w, pt, pl):
    """3x3 / s2 conv, ceil(size / 2) outputs, the window of output 0 starting pt rows and pl columns before the image"""
    H, W = x.shape[-2:]
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    return F.conv2d(F.pad(x, [pl, max((Wo - 1) * 2 + 3 - W - pl, 0), pt, max((Ho - 1) * 2 + 3 - H - pt, 0)]), w, stride=2)


def dw3(e, taps, edge=False):
    return F.conv2d(F.pad(e, [1, 1, 1, 1], mode='replicate') if edge else F.pad(e, [1, 1, 1, 1]), taps, groups=taps.shape[0])


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def ref(d, sym, defect=None, fused=True):
    """float64 NHWC maps: y (R64), e (the stem map), A1 = |s1| conv(|x|, |w|) and, fused, D = |s2| dwconv(|e|, |taps|);
    None when the defect cannot change this case"""
    x, w = d['x'].double(), d['w'].double()
    H, W = x.shape[-2:]
    pt, pl = pads(H, sym), pads(W, sym)
    edge = False
    if defect == DEFECTS[0]:
        if (pt, pl) == (pads(H, not sym), pads(W, not sym)):
            return None
        pt, pl = pads(H, not sym), pads(W, not sym)
    elif defect == DEFECTS[1]:
        if not fused:
            return None
        edge = True
    elif defect == DEFECTS[2]:
        x = x.clone()
        x[..., -1] = 0.0
    e = pr.silu64(stem_conv(x, w, pt, pl) * _ch(d['s1']) + _ch(d['t1']))
    out = dict(e=nhwc(e), A1=nhwc(stem_conv(x.abs(), w.abs(), pt, pl) * _ch(d['s1']).abs()))
    if fused:
        taps = d['taps'].double()
        out['y'] = nhwc(pr.silu64(dw3(e, taps, edge) * _ch(d['s2']) + _ch(d['t2'])))
        out['D'] = nhwc(dw3(e.abs(), taps.abs()) * _ch(d['s2']).abs())
    else:
        out['y'] = out['e']
    return out


def oracle_f32(d, sym, fused=True):
    """the same through oracle.model's float32 functions"""
    pad = '' if sym else 'same'
    e = om.silu(om.conv2d_pad(d['x'], d['w'], None, 2, pad) * d['s1'][None, :, None, None] + d['t1'][None, :, None, None])
    if not fused:
        return nhwc(e)
    return nhwc(om.silu(om.conv2d_pad(e, d['taps'], None, 1, pad, groups=e.shape[1]) * d['s2'][None, :, None, None] + d['t2'][None, :, None, None]))


def fused_bound(dtype, in_dtype, roll, d, r):
    """per-element bound on |got - R64| of a fused launch (module docstring), NHWC like R64"""
    top = float(r['y'].abs().max())
    if dtype == 0:
        return torch.full_like(r['y'], F32_TOL * top)
    if dtype == 2:
        return torch.full_like(r['y'], TOLP * top)
    n1 = (0 if in_dtype == 1 else 1) + (1 if roll else 0)
    de = SLOPE * n1 * U * r['A1'] + U * r['e'].abs()
    dz2 = nhwc(dw3(de.permute(0, 3, 1, 2), d['taps'].double().abs())) * d['s2'].double().abs()
    if roll:
        dz2 = dz2 + U * r['D']
    return SLOPE * dz2 + U * r['y'].abs() + F32_TOL * top


def unfused_bound(dtype, in_dtype, r):
    top = float(r['e'].abs().max())
    if dtype == 0:
        return torch.full_like(r['e'], F32_TOL * top)
    if dtype == 2:
        return torch.full_like(r['e'], TOLP * top)
    return SLOPE * (1 if in_dtype == 2 else 0) * U * r['A1'] + U * r['e'].abs() + F32_TOL * top


def _q(x, dtype):
    """float64 -> the nearest value the storage type holds"""
    x = x.float()
    if dtype == 2:                                                    # hi = bf16(x), lo = bf16(x - hi), any shape
        hi = x.bfloat16().float()
        return hi.double() + (x - hi).bfloat16().double()
    return pr.stored(x, dtype).double()


def emulate(dtype, in_dtype, roll, d, sym, fused=True):
    """float64 arithmetic with the roundings the form makes where it makes them (module docstring; float32 and two-term: the
    storage roundings of the operands, the stem map and the output) -> (the stored output, the value the pool sums add), NHWC"""
    x, w = d['x'].double(), d['w'].double()
    H, W = x.shape[-2:]
    pt, pl = pads(H, sym), pads(W, sym)
    if not fused:
        if dtype == 1 and in_dtype == 2:
            x = _q(x, 1)
        e = pr.silu64(stem_conv(x, w, pt, pl) * _ch(d['s1']) + _ch(d['t1']))
        return nhwc(_q(e, dtype)), None
    taps = d['taps'].double()
    x = _q(x, 0 if dtype == 0 else dtype)                             # the staged image: float32 | bf16 | hi + lo
    if roll:
        wf = _q(w * d['s1'].double()[:, None, None, None] * ESC, dtype)
        t = stem_conv(x, wf, pt, pl) + _ch(d['t1']) * ESC
        ring = _q(t / (torch.exp2(t) + 1.0), 1 if dtype == 1 else 0)  # -log2(e) silu(z1); the two-term ring holds float32
        tf = taps * d['s2'].double()[:, None, None, None] * EINV
        z2 = dw3(ring, _q(tf, 1) if dtype == 1 else tf.float().double()) + _ch(d['t2'])
    else:
        e = _q(pr.silu64(stem_conv(x, w, pt, pl) * _ch(d['s1']) + _ch(d['t1'])), dtype)
        z2 = dw3(e, taps) * _ch(d['s2']) + _ch(d['t2'])
    v = nhwc(pr.silu64(z2))
    y = _q(v, dtype)
    return y, (v if roll else y)


def pool_rows(y, p, drop_last=False):
    """y: [B, Ho, Wo, C] float64 -> [B, parts, C]: the sums over each part of the plan p, tiles row-major | band * nstrips + strip
    (drop_last: the defective sum that misses a part's last pixel)"""
    out = torch.zeros(y.shape[0], p['parts'], y.shape[3], dtype=torch.float64)
    for iy in range(p['ny']):
        for ix in range(p['nx']):
            part = y[:, iy * p['bh']:(iy + 1) * p['bh'], ix * p['bw']:(ix + 1) * p['bw']].reshape(y.shape[0], -1, y.shape[3])
            out[:, iy * p['nx'] + ix] = (part[:, :-1] if drop_last else part).sum(1)
    return out


def pool_bound(dtype, y, p):
    """_dwconv_cases.pool_bound's construction on the parts of the plan: bh x bw float32 values added in a fixed order; the rolling
    form adds the value before its final rounding (u of the stored value in bf16, 2^-16 in the two-term dtype)"""
    rep = (U if dtype == 1 else 2.0 ** -16 if dtype == 2 else 0.0) if p['roll'] else 0.0
    return ((p['bh'] * p['bw'] - 1) * 2.0 ** -24 + rep) * pool_rows(y.abs(), p) + 1e-30
