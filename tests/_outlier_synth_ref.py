"""numpy restatement of ood_synth.OutlierSynthesizer (csrc/outlier_synth.hip): Philox4x32-10 in uint64 arithmetic, the Box-Muller
normals, r2 = |eps|^2, the selection of the k largest and the rows mu + L eps - each in float64, and in float32 with the device's
order of every sum written out (one rounding per operation).

    counter = (j, c | q << 16, t_lo, t_hi), key = (seed_lo, seed_hi) for candidate j, class c, feature block q, draw t
    word x -> u1 = (float(x >> 8) + 1) 2^-24 in (0, 1],  u2 = float(x >> 8) 2^-24 in [0, 1)     (both exact in float32)
    words (0, 1) and (2, 3): z = sqrt(-2 log u1) cos(2 pi u2), sqrt(-2 log u1) sin(2 pi u2)      -> features 4 q .. 4 q + 3
    float32: r = sqrtf(-2 logf(u1)), a = fl(2 pi) * u2, r * cosf(a), r * sinf(a); float64: the same formulas on the same u in float64
    r2       float32: r2 = 0, r2 = r2 + z_d * z_d for d ascending;  float64: the sum
    select   r2 descending, equal r2 by j ascending, the first k
    rows     float32: acc = 0, acc = acc + L[d, d'] * eps_d' for d' = 0 .. d ascending, x_d = mu_d + acc;  float64: mu + L eps
    log_density = -r2 / 2 + log_const,  log_const = -sum log L_dd - F / 2 log(2 pi)"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 of broadcastable integer arrays -> four uint32 arrays."""
    c = [np.asarray(v, np.uint64) & MASK for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    m0, m1, s32 = np.uint64(M0), np.uint64(M1), np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]                     # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> s32) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> s32) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def words(seed, t, c, j, F):
    """The words of candidates j (array) of class c at draw t: uint32 [len(j), F]."""
    j = np.asarray(j, np.uint64)
    q = np.arange(F // 4, dtype=np.uint64)
    seed, t = int(seed) & (2 ** 64 - 1), int(t) & (2 ** 64 - 1)
    w = philox(j[:, None], np.uint64(c) | (q[None, :] << np.uint64(16)), t & 0xFFFFFFFF, t >> 32, seed & 0xFFFFFFFF, seed >> 32)
    return np.stack(w, -1).reshape(j.shape[0], F)


def normals(w, dtype):
    """Box-Muller of the words [n, F] (F a multiple of 4) in `dtype`: words (0, 1) and (2, 3) of a block are one pair."""
    T = np.dtype(dtype).type
    x, y = w[:, 0::2] >> np.uint32(8), w[:, 1::2] >> np.uint32(8)
    scale = T(2.0 ** -24)
    u1, u2 = (x.astype(T) + T(1.0)) * scale, y.astype(T) * scale
    r = np.sqrt(T(-2.0) * np.log(u1))
    a = T(2.0 * np.pi) * u2                               # float32: fl(2 pi), and the product rounded
    z = np.empty(w.shape, T)
    z[:, 0::2], z[:, 1::2] = r * np.cos(a), r * np.sin(a)
    return z


def sqnorm(z):
    """r2 of every row of z in z's dtype: float32 in the device's order (d ascending, product and sum rounded separately)."""
    if z.dtype == np.float64:
        return (z * z).sum(1)
    r2 = np.zeros(z.shape[0], np.float32)
    for d in range(z.shape[1]):
        r2 = r2 + z[:, d] * z[:, d]
    return r2


def select(r2, k):
    """The k largest, descending, equal values by the smaller index."""
    return np.argsort(-r2, kind='stable')[:k]


def rows(mu_c, L, eps):
    """mu_c [F] + L eps for eps [n, F], in eps's dtype; float32 in the device's order."""
    if eps.dtype == np.float64:
        return np.asarray(mu_c, np.float64)[None] + eps @ np.asarray(L, np.float64).T
    L32, mu32 = np.asarray(L, np.float64).astype(np.float32), np.asarray(mu_c, np.float64).astype(np.float32)
    F = L32.shape[0]
    acc = np.zeros(eps.shape, np.float32)
    for dp in range(F):                                   # output d takes the terms d' = 0 .. d, ascending
        acc[:, dp:] = acc[:, dp:] + L32[dp:, dp][None, :] * eps[:, dp:dp + 1]
    return mu32[None] + acc


def log_const(L):
    L = np.asarray(L, np.float64)
    return -float(np.log(L.diagonal()).sum()) - 0.5 * L.shape[0] * float(np.log(2.0 * np.pi))


def candidates(seed, t, classes, S, F):
    """-> (z64, z32) [n, S, F]: the normals of every candidate in both precisions, from the same words"""
    z64, z32 = [], []
    for c in classes:
        w = words(seed, t, c, np.arange(S), F)
        z64.append(normals(w, np.float64)); z32.append(normals(w, np.float32))
    return np.stack(z64), np.stack(z32)


def sample(seed, t, classes, S, F, k, mu, L, valid=None, dtype=np.float64, z=None):
    """One draw restated: dict(rows [n, k, F], index [n, k], r2, log_density [n, k], roles [n * k], r2_all [n, S])."""
    classes = list(classes)
    if z is None:
        z = candidates(seed, t, classes, S, F)[0 if np.dtype(dtype) == np.float64 else 1]
    T = z.dtype.type
    n = len(classes)
    out = {'rows': np.zeros((n, k, F), T), 'index': np.zeros((n, k), np.int32), 'r2': np.zeros((n, k), T),
           'roles': np.zeros(n * k, np.int8), 'r2_all': np.zeros((n, S), T)}
    for ci, c in enumerate(classes):
        r2 = sqnorm(z[ci])
        idx = select(r2, k)
        out['r2_all'][ci], out['index'][ci], out['r2'][ci] = r2, idx, r2[idx]
        if valid is None or valid[c]:
            out['rows'][ci] = rows(mu[c], L, z[ci][idx])
        else:
            out['roles'][ci * k:(ci + 1) * k] = -1
    cst = log_const(L)
    out['log_density'] = -(out['r2'] * T(0.5)) + T(cst)
    return out


def gaussians(F, C, seed, identity=False):
    """Random class means and a random well-conditioned lower factor (diagonal in [0.5, 1.5], small off-diagonal part), float64 values
    that are float32 numbers; identity: L = I."""
    g = np.random.default_rng(seed)
    mu = g.standard_normal((C, F)).astype(np.float32).astype(np.float64)
    if identity:
        return mu, np.eye(F)
    L = np.tril(g.standard_normal((F, F)) / np.sqrt(F), -1) + np.diag(g.uniform(0.5, 1.5, F))
    return mu, L.astype(np.float32).astype(np.float64)


def bound(e32, value):
    """The project's float32 bound: four times the float32 restatement's own error plus 1e-7 of the largest value."""
    return 4.0 * float(e32) + 1e-7 * float(np.abs(value).max())
