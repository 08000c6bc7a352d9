"""numpy restatement of ood_features.SubspaceFeatureOOD (csrc/feature_subspace.hip): the uploaded parameters and the scores.

`dtype=np.float64` is the reference.  `dtype=np.float32` is the yardstick: the parameters are formed in float64 by
`finalize_subspace` and rounded to float32 once, as the product uploads them (`params`), and BOTH forms start from those float32
values - so the eigen-solver's freedom is not part of any comparison - and evaluate in `dtype`, in the product's formula order

    xc = f - mu0 (bfloat16 widened exactly);  y = Rt xc;  r = sqrt(sum y^2);  pm = sum inv_lambda * y^2
    t = -logit_score for 'energy', logit_score for 'max_logit';  vim = t - (alpha * r): the product is rounded, then the difference

The float32 form's distance from the reference, E32, measures what float32 arithmetic costs on the inputs at hand; the device is
held to 4 * E32 + 1e-7 * max |value| per key (`bounds`)."""
import numpy as np

KEYS = ('residual', 'partial_mahalanobis', 'vim')


def inputs(F, n_fit, n_score, seed=0):
    """The seeded inputs of the GPU tests, in the style of `_feature_ood_ref.inputs`: a fixed orthogonal Q, scales
    geomspace(1, 0.1, F) (covariance condition 100), a mean 1.5 N(0, 1) + 0.75, features mu + g A^T rounded to float32; the "OOD"
    rows are the same draw plus unit noise; logit scores N(2, 3) rounded to float32.
    Returns dict(x_fit [n_fit, F], x_in, x_ood [n_score, F], logit [2 * n_score])."""
    rs = np.random.RandomState(7000 * F + seed)
    Q, _ = np.linalg.qr(rs.normal(size=(F, F)))
    A = Q * np.geomspace(1.0, 0.1, F)[None, :]
    mu = 1.5 * rs.normal(size=F) + 0.75
    xf = mu + rs.normal(size=(n_fit, F)) @ A.T
    xi = mu + rs.normal(size=(n_score, F)) @ A.T
    xo = xi + rs.normal(size=(n_score, F))
    logit = 2.0 + 3.0 * rs.normal(size=2 * n_score)
    return {'x_fit': xf.astype(np.float32), 'x_in': xi.astype(np.float32), 'x_ood': xo.astype(np.float32), 'logit': logit.astype(np.float32)}


def stats(x):
    """rows [n, F] (widened exactly) -> n_c [1], s_c [1, F], S [F, F] of one class"""
    x = np.asarray(x, np.float64)
    return np.array([len(x)], np.int64), x.sum(0)[None, :], x.T @ x


def params(p):
    """`finalize_subspace`'s dict -> the float32 values the product uploads: Rt [F - D, F], inv_lambda [F - D], mu0 [F]"""
    return {'Rt': np.ascontiguousarray(p['R'].T).astype(np.float32), 'inv_lambda': p['inv_lambda'].astype(np.float32),
            'mu0': p['mu0'].astype(np.float32)}


def widen_bf16(bits):
    """uint16 bfloat16 bits -> float32, exactly"""
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def score(x, q, dtype=np.float64, logit=None, alpha=None, negate=True):
    """rows x [n, F] float32 under the float32 parameters q (`params`), evaluated in `dtype` -> dict(r, residual,
    partial_mahalanobis [n] and, with logit [n] float32 and alpha, t and vim)"""
    Rt, il, mu0 = (q[k].astype(dtype) for k in ('Rt', 'inv_lambda', 'mu0'))
    xc = np.asarray(x, np.float32).astype(dtype) - mu0
    y = xc @ Rt.T
    y2 = y * y
    r = np.sqrt(y2.sum(1))
    out = {'r': r, 'residual': -r, 'partial_mahalanobis': -(il[None, :] * y2).sum(1)}
    if logit is not None and alpha is not None:
        t = np.asarray(logit, np.float32).astype(dtype)
        t = -t if negate else t
        ar = np.dtype(dtype).type(alpha) * r                    # one rounding
        out['t'], out['vim'] = t, t - ar                          # the second
    return out


def bounds(ref, f32):
    """key -> (E32, bound): E32 = the float32 restatement's largest error on that key; bound = 4 E32 + 1e-7 max |value|"""
    out = {}
    for k in KEYS:
        if k in ref:
            e32 = float(np.abs(f32[k].astype(np.float64) - ref[k]).max())
            out[k] = (e32, 4.0 * e32 + 1e-7 * float(np.abs(ref[k]).max()))
    return out
