"""numpy restatement of ood_features.KNNFeatureOOD (csrc/feature_knn.hip): the bank bookkeeping (`Bank`), the normalisation, the
squared distance d2 = max((|q|^2 + |r|^2) - 2 q.r, 0) in the stated order, the k-th smallest and the nearest row by (d2, i).

`dtype=np.float64` is the reference.  `dtype=np.float32` is the yardstick: every step above evaluated in float32 (|x|^2 in the
product's summation order, the dot products by numpy's float32 matmul).  Its distance from the reference, E32, measures what
float32 arithmetic costs on the inputs at hand; the device is held to 4 * E32 + 1e-7 * max d2 (`bound`), both terms taken from
the restatement, never from the device.  The nearest row is compared exactly outside the rows whose float64 gap between the
nearest and the second-nearest d2 is at most twice that bound (`excluded`)."""
import numpy as np


def inputs(F, C, n_bank, n_q, seed=0):
    """The seeded inputs of the tests: a fixed orthogonal Q, scales geomspace(1, 0.1, F), class means 1.5 N(0, 1) + 0.75, features
    mu_y + g A^T rounded to float32; the "OOD" rows are the query draw plus unit noise.
    Returns dict(x_bank [n_bank, F], y_bank, x_in [n_q, F], y_in, x_ood [n_q, F])."""
    rs = np.random.RandomState(1000 * F + C + seed)
    Q, _ = np.linalg.qr(rs.normal(size=(F, F)))
    A = Q * np.geomspace(1.0, 0.1, F)[None, :]
    mu = 1.5 * rs.normal(size=(C, F)) + 0.75
    yb, yq = rs.randint(0, C, n_bank), rs.randint(0, C, n_q)
    xb = mu[yb] + rs.normal(size=(n_bank, F)) @ A.T
    xq = mu[yq] + rs.normal(size=(n_q, F)) @ A.T
    xo = xq.astype(np.float32) + rs.normal(size=(n_q, F))
    return {'x_bank': xb.astype(np.float32), 'y_bank': yb.astype(np.int64), 'x_in': xq.astype(np.float32), 'y_in': yq.astype(np.int64),
            'x_ood': xo.astype(np.float32)}


def sumsq(x, dtype=np.float64):
    """|x|^2 per row in the product's order: 16 partial sums over k mod 16 (k ascending), then the tree (p[j] + p[j + 8]),
    (.. + 4), (.. + 2), (.. + 1); one rounding per operation in `dtype`"""
    x = np.asarray(x).astype(dtype)
    n, F = x.shape
    Fp = -(-F // 16) * 16
    xp = np.zeros((n, Fp), dtype)
    xp[:, :F] = x
    p = np.zeros((n, 16), dtype)
    for c in range(0, Fp, 16):
        p = p + xp[:, c:c + 16] * xp[:, c:c + 16]
    u = p[:, :8] + p[:, 8:]
    v = u[:, :4] + u[:, 4:]
    return (v[:, 0] + v[:, 2]) + (v[:, 1] + v[:, 3])


def stored(x, normalize, dtype=np.float64):
    """rows as the bank stores them (and as a query enters the distance) -> (rows [n, F], |row|^2 [n]) in `dtype`"""
    x = np.asarray(x).astype(dtype)
    if normalize:
        t = np.dtype(dtype).type
        inv = t(1) / np.sqrt(np.maximum(sumsq(x, dtype), t(1e-24)))
        x = x * inv[:, None]
    return x, sumsq(x, dtype)


def distances(q, bank, normalize, dtype=np.float64):
    """d2 [n_q, M] of raw query rows against raw bank rows, in `dtype`"""
    t = np.dtype(dtype).type
    qs, qn = stored(q, normalize, dtype)
    bs, bn = stored(bank, normalize, dtype)
    return np.maximum((qn[:, None] + bn[None, :]) - t(2) * (qs @ bs.T), t(0))


def select(d2, k, classes=None):
    """-> dict(knn = -(k_eff-th smallest), index = argmin by (d2, i), cls, gap = second smallest - smallest (inf when M = 1))"""
    M = d2.shape[1]
    at = sorted({0, min(1, M - 1), min(k, M) - 1})
    part = np.partition(d2, at, 1)
    index = d2.argmin(1)                                     # the first of equal values: the lower row
    gap = part[:, 1] - part[:, 0] if M > 1 else np.full(d2.shape[0], np.inf)
    cls = np.full(d2.shape[0], -1, np.int64) if classes is None else np.asarray(classes, np.int64)[index]
    return {'knn': -part[:, min(k, M) - 1], 'index': index, 'cls': cls, 'gap': gap, 'max_d2': float(d2.max()) if d2.size else 0.0}


def score(q, bank, k, normalize, classes=None, dtype=np.float64):
    return select(distances(q, bank, normalize, dtype), k, classes)


def bound(ref, f32):
    """(E32, bound): E32 = the float32 restatement's largest |knn| error; bound = 4 E32 + 1e-7 max d2 (float64 restatement)"""
    e32 = float(np.abs(f32['knn'].astype(np.float64) - ref['knn']).max())
    return e32, 4.0 * e32 + 1e-7 * ref['max_d2']


def excluded(ref, value_bound):
    """rows whose nearest and second-nearest bank row are within twice the value bound of each other in the reference"""
    return ref['gap'] <= 2.0 * value_bound


class Bank:
    """The bookkeeping of `effdet_feature_knn_append`: valid rows arrive in order; the one with global ordinal g (since clear) is
    kept when g % sample_every == 0; kept rows beyond the capacity are dropped and counted."""

    def __init__(self, F, capacity, normalize=True, sample_every=1, dtype=np.float32):
        self.F, self.capacity, self.normalize, self.every, self.dtype = F, capacity, normalize, sample_every, dtype
        self.clear()

    def clear(self):
        self.rows = np.zeros((0, self.F), self.dtype)
        self.norms = np.zeros(0, self.dtype)
        self.classes = np.zeros(0, np.int64)
        self.seen = self.lost = 0

    size = property(lambda self: self.rows.shape[0])

    def add(self, x, y=None):
        x = np.asarray(x)
        n = x.shape[0]
        y = np.full(n, -1, np.int64) if y is None else np.asarray(y, np.int64)
        keep = (self.seen + np.arange(n)) % self.every == 0
        self.seen += n
        x, y = x[keep], y[keep]
        room = self.capacity - self.size
        self.lost += max(x.shape[0] - room, 0)
        x, y = x[:room], y[:room]
        rows, norms = stored(x, self.normalize, self.dtype)
        self.rows = np.concatenate([self.rows, rows.astype(self.dtype)])
        self.norms = np.concatenate([self.norms, norms.astype(self.dtype)])
        self.classes = np.concatenate([self.classes, y])


KS = (1, 5, 32)
N_BANK, N_Q = 4096, 2000
_CASES = {}


def case(F, C, normalize):
    """The shared case of the host and GPU tests, computed once and left unchanged: inputs(F, C, 4096, 2000), the queries the in
    rows followed by the OOD rows, and per k in KS the float64 restatement, E32 and the bound over all 4000 queries."""
    key = (F, C, bool(normalize))
    if key not in _CASES:
        d = inputs(F, C, N_BANK, N_Q)
        q = np.concatenate([d['x_in'], d['x_ood']])
        d64 = distances(q, d['x_bank'], normalize)
        d32 = distances(q, d['x_bank'], normalize, np.float32)
        out = {'d': d, 'q': q}
        for k in KS:
            ref, f32 = select(d64, k, d['y_bank']), select(d32, k)
            out[k] = (ref,) + bound(ref, f32)
        _CASES[key] = out
    return _CASES[key]
