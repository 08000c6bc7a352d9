"""numpy restatement of ood_features.FeatureOOD: fit (n_c, s_c, S), finalize (whitening factors, class means) and score.

`dtype=np.float64` is the reference.  `dtype=np.float32` is the yardstick: the parameters are formed in float64 and rounded to
float32 once, as the product uploads them, and the score is evaluated in float32 in the product's formula order
(xc = f - mu0; z = W xc; q = sum z^2; d_c = (q - 2 z.M_c) + |M_c|^2).  Its distance from the reference, E32, measures what
float32 arithmetic costs on the inputs at hand; the device is held to 4 * E32 + 1e-7 * max |d| (`score_bound`)."""
import numpy as np


def inputs(F, C, n_fit, n_score, seed=0):
    """The seeded inputs of the GPU tests: a fixed orthogonal Q, scales geomspace(1, 0.1, F) (covariance condition 100), class
    means 1.5 N(0, 1) + 0.75, features mu_y + g A^T rounded to float32; the "OOD" rows are the same draw plus unit noise.
    Returns dict(x_fit [n_fit, F], y_fit [n_fit], x_in, y_in, x_ood [n_score, F])."""
    rs = np.random.RandomState(1000 * F + C + seed)
    Q, _ = np.linalg.qr(rs.normal(size=(F, F)))
    A = Q * np.geomspace(1.0, 0.1, F)[None, :]
    mu = 1.5 * rs.normal(size=(C, F)) + 0.75

    def draw(n):
        y = rs.randint(0, C, n)
        return (mu[y] + rs.normal(size=(n, F)) @ A.T), y
    xf, yf = draw(n_fit)
    xi, yi = draw(n_score)
    xo = xi + rs.normal(size=(n_score, F))
    return {'x_fit': xf.astype(np.float32), 'y_fit': yf.astype(np.int64), 'x_in': xi.astype(np.float32), 'y_in': yi.astype(np.int64),
            'x_ood': xo.astype(np.float32)}


def fit(x, y, C):
    """rows x [n, F] (any float dtype, widened exactly) with classes y [n]; rows with a class outside [0, C) are skipped"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.int64)
    ok = (y >= 0) & (y < C)
    x, y = x[ok], y[ok]
    n_c = np.bincount(y, minlength=C).astype(np.int64)
    s_c = np.zeros((C, x.shape[1]))
    np.add.at(s_c, y, x)
    return n_c, s_c, x.T @ x


def finalize(n_c, s_c, S, shrinkage=0.0):
    """float64: mu_c, tied covariance, pooled mean / covariance, W = L^-1, W0 = L0^-1, M_c = W (mu_c - mu_0), |M_c|^2"""
    n_c = np.asarray(n_c, np.int64)
    C, F = s_c.shape
    n = float(n_c.sum())
    have = n_c > 0
    mu = np.zeros((C, F))
    mu[have] = s_c[have] / n_c[have, None]
    cov = S.copy()
    for c in np.nonzero(have)[0]:
        cov -= n_c[c] * np.outer(mu[c], mu[c])
    cov /= n
    mu0 = s_c.sum(0) / n
    cov0 = S / n - np.outer(mu0, mu0)
    if shrinkage:
        cov = cov + shrinkage * np.trace(cov) / F * np.eye(F)
        cov0 = cov0 + shrinkage * np.trace(cov0) / F * np.eye(F)
    W = np.linalg.inv(np.linalg.cholesky(cov))
    W0 = np.linalg.inv(np.linalg.cholesky(cov0))
    M = (mu - mu0) @ W.T
    m2 = np.where(have, (M * M).sum(1), np.inf)
    return {'mu': mu, 'mu0': mu0, 'cov': cov, 'cov0': cov0, 'W': W, 'W0': W0, 'M': M, 'm2': m2, 'have': have}


def score(x, p, dtype=np.float64):
    """-> dict(d [n, C] (inf for empty classes), d0 [n], mahalanobis, relative [n], nearest [n]) evaluated in `dtype`"""
    t = np.dtype(dtype).type
    W, W0, M, mu0 = (p[k].astype(dtype) for k in ('W', 'W0', 'M', 'mu0'))
    m2 = p['m2'].astype(dtype)
    xc = np.asarray(x).astype(dtype) - mu0
    z, z0 = xc @ W.T, xc @ W0.T
    q, d0 = (z * z).sum(1), (z0 * z0).sum(1)
    d = (q[:, None] - t(2) * (z @ M.T)) + m2[None, :]
    d[:, ~p['have']] = np.inf
    dmin = d.min(1)
    return {'d': d, 'd0': d0, 'mahalanobis': -dmin, 'relative': -(dmin - d0), 'nearest': d.argmin(1)}


def score_bound(ref, f32):
    """(E32, bound): E32 = the float32 restatement's largest error over mahalanobis and relative; bound = 4 E32 + 1e-7 max |d|"""
    e32 = max(np.abs(f32[k].astype(np.float64) - ref[k]).max() for k in ('mahalanobis', 'relative'))
    finite = ref['d'][np.isfinite(ref['d'])]
    big = max(np.abs(finite).max(), np.abs(ref['d0']).max())
    return e32, 4.0 * e32 + 1e-7 * big


def near_ties(ref, bound):
    """rows whose best and second-best class are within twice the bound in the reference (none on the seeded inputs)"""
    d = np.sort(ref['d'], 1)
    if d.shape[1] < 2:
        return np.zeros(d.shape[0], bool)
    return (d[:, 1] - d[:, 0]) <= 2.0 * bound
