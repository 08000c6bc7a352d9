"""numpy restatement of ood_shaping.ActivationShapingOOD (csrc/act_shaping.hip): the penultimate row, the shaping, the scores and
the fit rules.

The penultimate row d is ALWAYS float32 by the stated steps - d_j = t_0j x_0j, then d_j = d_j + t_kj x_kj for k = 1 .. 8, every
product and every sum rounded once, x = 0 outside the map - and the device's d is bit-equal to it (the selections compare its
values).  Everything after d takes `dtype`: np.float64 is the reference, np.float32 the yardstick - the same formulas evaluated in
float32 from the same float32 inputs.  Its distance from the reference, E32, measures what float32 arithmetic costs on the inputs
at hand; the device is held to 4 * E32 + 1e-7 * max |value| per key (`bounds`).

    shaping (k = F - round(F * percentile / 100); kept = the k largest d_j by value, equal values to the lower j first;
             s1 = sum_j max(d_j, 0), s2 = the same over the kept set, f = exp(s1 / s2), 1 where s2 == 0):
      none x' = d;  react x' = min(d, c);  ash_p kept d_j, others 0;  ash_b kept s1 / k, others 0;  ash_s kept d_j f, others 0;
      scale d_j f for every j
    z_c = bias[a C + c] + sum_j W[a C + c][j] x'_j,  u = z / T:  energy = -T logsumexp(u),  max_logit = max z,  class = lowest argmax,
    gradnorm = (sum_c |softmax(z(d))_c - 1 / C|) * (sum_j |d_j|) from the unshaped row at T = 1
    a row with a non-finite d_j: NaN, NaN, -1, NaN"""
import math

import numpy as np

METHODS = ('none', 'react', 'ash_p', 'ash_b', 'ash_s', 'scale')
FLOAT_KEYS = ('energy', 'max_logit', 'gradnorm')
LEVELS = ((4, 3), (2, 2), (1, 1))       # the 1 x 1 level has every neighbour outside the map, the 3-wide one both edges


def silu(x):
    return x / (1.0 + np.exp(-x))


def inputs(F, C, A, B, levels=LEVELS, seed=0):
    """The seeded inputs of the tests: tower values silu(N(0, 1)) as per-level NHWC arrays [B, h, w, F], taps N(0, 0.3) [9, F],
    weights N(0, 1 / sqrt(F)) [A * C, F] with + 1 / sqrt(F) on one class of every anchor slot (wide arg-max margins), bias
    N(0, 0.1) [A * C]; all float32."""
    rs = np.random.RandomState(7000 + 13 * F + 101 * C + 3 * A + 17 * B + seed)
    tower = [silu(rs.normal(size=(B, h, w, F))).astype(np.float32) for h, w in levels]
    taps = rs.normal(0, 0.3, size=(9, F)).astype(np.float32)
    W = rs.normal(0, 1.0 / math.sqrt(F), size=(A * C, F))
    W[np.arange(A) * C + rs.randint(0, C, A)] += 1.0 / math.sqrt(F)
    bias = rs.normal(0, 0.1, size=A * C)
    return {'tower': tower, 'taps': taps, 'W': W.astype(np.float32), 'bias': bias.astype(np.float32)}


def to_bf16_bits(x):
    """float32 -> uint16 bfloat16 bits, round to nearest even (finite inputs)"""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def widen_bf16(bits):
    """uint16 bfloat16 bits -> float32, exactly"""
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def penultimate(tower, taps):
    """per-level NHWC float32 arrays, taps [9, F] -> d [B, P, F] float32 by the stated steps (cells level after level, y * w + x)"""
    taps = np.asarray(taps, np.float32)
    out = []
    for x in tower:
        x = np.asarray(x, np.float32)
        B, h, w, F = x.shape
        pad = np.zeros((B, h + 2, w + 2, F), np.float32)
        pad[:, 1:-1, 1:-1] = x
        d = None
        for k in range(9):
            ky, kx = divmod(k, 3)
            pr = taps[k][None, None, None, :] * pad[:, ky:ky + h, kx:kx + w]
            d = pr if d is None else d + pr
            assert d.dtype == np.float32
        out.append(d.reshape(B, h * w, F))
    return np.concatenate(out, 1)


def k_of(F, percentile):
    """entries kept by the ASH forms and SCALE: F - round(F * percentile / 100) (Python's round), which must lie in [1, F]"""
    k = int(F) - int(round(F * float(percentile) / 100.0))
    if not 1 <= k <= F:
        raise ValueError('percentile %r keeps %d of %d entries: k must lie in [1, F]' % (percentile, k, F))
    return k


def kept_set(d, k):
    """bool [n, F]: the k largest by value, equal values (-0 = +0) to the lower j first"""
    d = np.asarray(d, np.float32)
    order = np.argsort(-d, axis=1, kind='stable')[:, :k]
    kept = np.zeros(d.shape, bool)
    kept[np.arange(d.shape[0])[:, None], order] = True
    return kept


def shape(d, method, k=None, c=None, dtype=np.float64):
    """rows d [n, F] float32 (finite) -> x' [n, F] in `dtype`"""
    d = np.asarray(d, np.float32)
    x = d.astype(dtype)
    if method == 'none':
        return x
    if method == 'react':
        return np.minimum(x, dtype(np.float32(c)))
    kept = kept_set(d, k)
    pos = np.maximum(x, 0)
    s1 = pos.sum(1, dtype=dtype)
    s2 = np.where(kept, pos, 0).sum(1, dtype=dtype)
    with np.errstate(over='ignore'):
        f = np.where(s2 == 0, dtype(1), np.exp(s1 / np.where(s2 == 0, dtype(1), s2))).astype(dtype)
    if method == 'ash_p':
        return np.where(kept, x, 0)
    if method == 'ash_b':
        return np.where(kept, (s1 / dtype(k))[:, None], 0).astype(dtype)
    if method == 'ash_s':
        return np.where(kept, x * f[:, None], 0).astype(dtype)
    if method == 'scale':
        return (x * f[:, None]).astype(dtype)
    raise ValueError(method)


def logits(x, slots, W, bias, A, dtype=np.float64):
    """z [n, C] of rows x [n, F] (`dtype`) at the anchor slots `slots` [n]"""
    C = W.shape[0] // A
    Wr = np.asarray(W, np.float32).astype(dtype).reshape(A, C, -1)
    br = np.asarray(bias, np.float32).astype(dtype).reshape(A, C)
    slots = np.asarray(slots, np.int64)
    x = x.astype(dtype)
    z = np.zeros((len(x), C), dtype)
    for a in range(A):
        m = slots == a
        z[m] = br[a] + np.einsum('cf,if->ic', Wr[a], x[m])
    return z


def lse(u, dtype):
    m = u.max(1)
    return m + np.log(np.exp(u - m[:, None]).sum(1, dtype=dtype))


def score(d, slots, W, bias, A, method='none', k=None, c=None, T=1.0, gradnorm=False, dtype=np.float64):
    """rows d [n, F] float32 with their anchor slots [n] -> dict(energy, max_logit, class, rows (x'), logits, margin (the top two
    logits' difference) and gradnorm when asked), evaluated in `dtype`; rows with a non-finite d_j: NaN, NaN, -1, NaN"""
    d = np.asarray(d, np.float32)
    slots = np.asarray(slots, np.int64)
    fin = np.isfinite(d).all(1)
    dz = np.where(fin[:, None], d, np.float32(0))
    with np.errstate(all='ignore'):
        x = shape(dz, method, k, c, dtype)
        z = logits(x, slots, W, bias, A, dtype)
        C = z.shape[1]
        Tt = dtype(np.float32(T))
        out = {'energy': -(Tt * lse(z / Tt, dtype)), 'max_logit': z.max(1), 'class': z.argmax(1).astype(np.int64), 'rows': x, 'logits': z}
        if C > 1:
            part = np.partition(z, C - 2, axis=1)
            out['margin'] = part[:, C - 1] - part[:, C - 2]
        else:
            out['margin'] = np.full(len(d), np.inf)
        if gradnorm:
            z0 = logits(dz.astype(dtype), slots, W, bias, A, dtype)
            p = np.exp(z0 - lse(z0, dtype)[:, None])
            out['gradnorm'] = np.abs(p - dtype(1) / dtype(C)).sum(1, dtype=dtype) * np.abs(dz.astype(dtype)).sum(1, dtype=dtype)
    for key in out:
        if key == 'class':
            out[key] = np.where(fin, out[key], -1)
        elif key == 'margin':
            out[key] = np.where(fin, out[key], np.inf)
        else:
            out[key] = np.where(fin.reshape((-1,) + (1,) * (out[key].ndim - 1)), out[key], np.nan).astype(dtype)
    return out


def bounds(ref, f32, keys=FLOAT_KEYS + ('logits',)):
    """key -> (E32, bound): E32 = the float32 restatement's largest error on that key over the finite rows; bound = 4 E32 +
    1e-7 max |value|"""
    out = {}
    for key in keys:
        if key in ref:
            ok = np.isfinite(ref[key])
            e32 = float(np.abs(f32[key].astype(np.float64) - ref[key])[ok].max()) if ok.any() else 0.0
            out[key] = (e32, 4.0 * e32 + 1e-7 * float(np.abs(ref[key][ok]).max() if ok.any() else 0.0))
    return out


# ---- the fit rules -----------------------------------------------------------------------------------------------------------------
def key_of(d):
    """float32 -> uint32 whose unsigned order is the order of the floats"""
    b = np.ascontiguousarray(d, np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b ^ np.uint32(0x80000000)).astype(np.uint32)


def unkey(key):
    key = np.asarray(key, np.uint32)
    return np.where(key & np.uint32(0x80000000), key ^ np.uint32(0x80000000), ~key).astype(np.uint32).view(np.float32)


def fit_stats(d):
    """finite rows of d [n, F] float32 -> n, sum_d [F] float64, hist [65536] int64 over the upper 16 key bits of every d_j"""
    d = np.asarray(d, np.float32)
    d = d[np.isfinite(d).all(1)]
    return len(d), d.astype(np.float64).sum(0), np.bincount((key_of(d) >> 16).ravel(), minlength=65536).astype(np.int64)


def react_threshold(hist, n, F, percentile):
    """the largest finite float32 whose key falls into the first bin at which the cumulative count reaches
    ceil(percentile / 100 * n * F) (at least 1) -> (c as float32, the bin)"""
    hist = np.asarray(hist, np.int64)
    if n < 1 or int(hist.sum()) != n * F:
        raise ValueError('the histogram holds %d values, not n * F = %d * %d (n >= 1)' % (int(hist.sum()), n, F))
    target = max(int(math.ceil(float(percentile) / 100.0 * (n * F))), 1)
    b = int(np.searchsorted(np.cumsum(hist), target, side='left'))
    c = unkey(np.uint32((b << 16) | 0xFFFF)).reshape(())
    if not np.isfinite(c):                                      # (the bins of -inf and of the NaN patterns hold no finite value)
        raise ValueError('bin %d holds no finite float32' % b)
    return np.float32(c), b


def dice_weight(W, sum_d, n, p):
    """W [A * C, F] float32 with the entries whose contribution V = W * (sum_d / n) lies at or below the p-th percentile of V set
    to 0 (numpy percentile, default interpolation, float64) -> (the masked float32 weight, the bool mask of the kept entries)"""
    V = np.asarray(W, np.float32).astype(np.float64) * (np.asarray(sum_d, np.float64) / float(n))[None, :]
    keep = V > np.percentile(V, float(p))
    return np.where(keep, np.asarray(W, np.float32), np.float32(0)), keep
