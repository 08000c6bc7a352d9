"""numpy restatement of ood_logits.LogitOOD (csrc/logit_ood.hip): the statistics of a fit and the scores.

`dtype=np.float64` is the reference.  `dtype=np.float32` is the yardstick: the same formulas in the product's operation order,
evaluated in float32 from the SAME float32 inputs (the logits, the temperature and gamma rounded to float32, and the float32
log D / kl_inf / mu / inv_sigma the product uploads, `params`).  With a row z of C logits and u = z / T:

    m = max u, k* = argmax (the lowest index among ties);  e_k = exp(u_k - m), s = sum e, lse = m + log s, l_k = u_k - lse, p_k = exp(l_k)
    msp = exp(m - lse);  neg_entropy = sum p_k l_k
    gen = -sum over the top_m largest u_k (stable: the lower k first among equals) of exp(gamma (l_k + q_k)),
          q_k = log1p(-p_k) for k != k*,  q_k* = log(sum_{k != k*} e_k) - log s   (-inf at C = 1: the term is 0)
    joint_energy = sum max(z_k, 0) + log1p(exp(-|z_k|))
    kl_c = (neg_entropy - sum_k p_k log D_ck) + kl_inf_c  with p and neg_entropy at T = 1;  kl_matching = -min_c kl_c;  kl_class = argmin
    standardized_max_logit = (max z - mu_k*) * inv_sigma_k*

The float32 form's distance from the reference, E32, measures what float32 arithmetic costs on the inputs at hand; the device is
held to 4 * E32 + 1e-7 * max |value| per key (`bounds`)."""
import numpy as np

KEYS = ('msp', 'neg_entropy', 'gen', 'joint_energy', 'predicted_class', 'kl_matching', 'kl_class', 'standardized_max_logit')
FLOAT_KEYS = ('msp', 'neg_entropy', 'gen', 'joint_energy', 'kl_matching', 'standardized_max_logit')
FITTED_KEYS = ('kl_matching', 'kl_class', 'standardized_max_logit')


def inputs(C, n_fit=2048, n_score=500, seed=0):
    """The seeded inputs of the tests: logits 2 N(0, 1) - 3 with +5 on one random class of every in-distribution row and +1 on one
    of every "OOD" row, rounded to float32.  Returns dict(z_fit [n_fit, C], z_in, z_ood [n_score, C])."""
    rs = np.random.RandomState(9000 + 31 * C + seed)

    def draw(n, boost):
        z = 2.0 * rs.normal(size=(n, C)) - 3.0
        z[np.arange(n), rs.randint(0, C, n)] += boost
        return z.astype(np.float32)
    return {'z_fit': draw(n_fit, 5.0), 'z_in': draw(n_score, 5.0), 'z_ood': draw(n_score, 1.0)}


def widen_bf16(bits):
    """uint16 bfloat16 bits -> float32, exactly"""
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def softmax(z, T=1.0, dtype=np.float64):
    """rows z [n, C] float32 -> dict(u, m, kstar, e, s, lse, l, p) in `dtype`"""
    u = np.asarray(z, np.float32).astype(dtype) / dtype(np.float32(T))
    m = u.max(1)
    e = np.exp(u - m[:, None])
    s = e.sum(1, dtype=dtype)
    lse = m + np.log(s)
    l = u - lse[:, None]
    return {'u': u, 'm': m, 'kstar': u.argmax(1), 'e': e, 's': s, 'lse': lse, 'l': l, 'p': np.exp(l)}


def stats(z, C, T=1.0, dtype=np.float64):
    """rows -> n_c [C] int64, P_c [C, C], a_c, b_c [C] float64: per predicted class (the argmax of u = z / T) the number of rows,
    the sum of p at T = 1 (evaluated in `dtype`), of max z and of (max z)^2"""
    z = np.asarray(z, np.float32)
    ks = softmax(z, T, dtype)['kstar']
    p = softmax(z, 1.0, dtype)['p'].astype(np.float64)
    mz = z.max(1).astype(np.float64)
    n_c, P_c, a_c, b_c = np.zeros(C, np.int64), np.zeros((C, C)), np.zeros(C), np.zeros(C)
    np.add.at(n_c, ks, 1)
    np.add.at(P_c, ks, p)
    np.add.at(a_c, ks, mz)
    np.add.at(b_c, ks, mz * mz)
    return n_c, P_c, a_c, b_c


def params(p):
    """`ood_logits.finalize`'s dict -> the float32 values the product uploads (without the tile padding)"""
    return {k: p[k].astype(np.float32) for k in ('log_d', 'kl_inf', 'mu', 'inv_sigma')}


def score(z, dtype=np.float64, T=1.0, gamma=0.1, top_m=10, q=None):
    """rows z [n, C] float32, evaluated in `dtype` -> dict of [n] arrays: the keys, and with the float32 parameters q (`params`)
    the fitted keys, `kl` [n, C] and `kl_margin` (the second-best kl minus the best)"""
    z = np.asarray(z, np.float32)
    n, C = z.shape
    rows = np.arange(n)
    sm = softmax(z, T, dtype)
    u, ks, e, s, l, p = sm['u'], sm['kstar'], sm['e'], sm['s'], sm['l'], sm['p']
    out = {'predicted_class': ks.astype(np.int64), 'msp': np.exp(sm['m'] - sm['lse']), 'neg_entropy': (p * l).sum(1, dtype=dtype)}
    eo = e.copy()
    eo[rows, ks] = 0
    with np.errstate(divide='ignore'):
        qs = np.log(eo.sum(1, dtype=dtype)) - np.log(s)
        qk = np.log1p(-p)                                       # (p_k* may round to 1: replaced below)
    qk[rows, ks] = qs
    term = np.exp(dtype(np.float32(gamma)) * (l + qk))
    m_ = min(int(top_m), C)
    order = np.argsort(-u, axis=1, kind='stable')[:, :m_]
    sel = np.zeros((n, C), bool)
    sel[rows[:, None], order] = True
    out['gen'] = -np.where(sel, term, 0).sum(1, dtype=dtype)
    zd = z.astype(dtype)
    out['joint_energy'] = (np.maximum(zd, 0) + np.log1p(np.exp(-np.abs(zd)))).sum(1, dtype=dtype)
    if q is not None:
        s1 = softmax(z, 1.0, dtype)
        ne1 = (s1['p'] * s1['l']).sum(1, dtype=dtype)
        kl = (ne1[:, None] - s1['p'] @ q['log_d'].astype(dtype).T) + q['kl_inf'].astype(dtype)[None, :]
        kc = kl.argmin(1)
        out['kl'], out['kl_class'], out['kl_matching'] = kl, kc.astype(np.int64), -kl[rows, kc]
        if C > 1:
            part = np.partition(kl, 1, axis=1)
            out['kl_margin'] = part[:, 1] - part[:, 0]
        else:
            out['kl_margin'] = np.full(n, np.inf)
        d = z.max(1).astype(dtype) - q['mu'].astype(dtype)[ks]
        out['standardized_max_logit'] = d * q['inv_sigma'].astype(dtype)[ks]
    return out


def bounds(ref, f32):
    """key -> (E32, bound): E32 = the float32 restatement's largest error on that key; bound = 4 E32 + 1e-7 max |value|"""
    out = {}
    for k in FLOAT_KEYS:
        if k in ref:
            e32 = float(np.abs(f32[k].astype(np.float64) - ref[k]).max())
            out[k] = (e32, 4.0 * e32 + 1e-7 * float(np.abs(ref[k]).max()))
    return out
