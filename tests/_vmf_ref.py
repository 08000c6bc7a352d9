"""numpy restatement of ood_vmf.VMFHead / VMFFeatureOOD (csrc/vmf.hip): the vMF partition function, the ordered prototype update,
the loss with its analytic gradients, and the scores.

`dtype=np.float64` is the reference.  `dtype=np.float32` is the yardstick: the same formulas in the product's operation order, the
per-row terms in float32 from the SAME float32 inputs and the sums over rows in float64, as the product adds them.

    entry i = (b, j) of a dense [B, K = A P] label map counts when its label y lies in [0, C) and the row u of its cell p = j // A
    (a row of U [B, P, d] float32) holds finite values only; for the loss its class must be valid as well
    n = max(sqrt(sum u_k^2), 1e-12), r = u / n                       the sum in `row_sum` order
    kappa_c = float32(exp(clamp(theta_c, log 2^-7, log 2^13))), nu = d / 2 - 1
    logZ_c = nu log kappa_c - (d / 2) log(2 pi) - log I_nu(kappa_c),  A_c = I_{nu+1}(kappa_c) / I_nu(kappa_c)      (float64, `bessel`)
    l_c = float32(logZ_c) + kappa_c (mu_c . r)                       valid classes only; the dot product adds k = 0 .. d - 1 in order
    loss_i = logsumexp_c l_c - l_y,  p = softmax l,  g_c = (p_c - [c = y]) * dtype(1 / max(m, 1))
    loss = (1 / max(m, 1)) sum_i loss_i                              (float64 sum)
    d theta_c = kappa_c sum_i g_ic ((mu_c . r_i) - A_c)              (float64 terms and sum; 0 where the clamp is active)
    G = sum_c (g_c kappa_c) mu_c  (c ascending),  du = (G - (G . r) r) / n;  dU of a cell: its counted anchors' du added ascending
    update    per class, its counted rows in (b, j) order, at most `limit`: v = alpha mu + (1 - alpha) r, mu = v / max(|v|, 1e-12),
              float32, one rounding per operation, the norm in `row_sum` order; the class is valid afterwards
    scores    vmf = max_c l_c, vmf_class the lowest class that attains it, vmf_cosine = max_c mu_c . r (valid classes)

The float32 form's distance from the reference, E32, measures what float32 arithmetic costs on the inputs at hand; the device is
held to 4 * E32 + 1e-7 * max |value| per key (`bound`)."""
import math

import numpy as np

EPS = 1e-12
THETA_LO, THETA_HI = np.float32(math.log(2.0 ** -7)), np.float32(math.log(2.0 ** 13))
LOG_2PI = 1.8378770664093453
KEYS = ('vmf', 'vmf_class', 'vmf_cosine')


def bessel(nu, x):
    """-> (log I_nu(x), I_{nu+1}(x) / I_nu(x)) for x > 0, nu >= 0, python floats.  I_nu(x) = (x / 2)^nu sum_k q^k / (k! Gamma(nu + k + 1))
    with q = x^2 / 4: positive terms, taken relative to the largest one k0 (the root of k (nu + k) = q) and added from it upwards and
    then downwards by the term ratio until a term is below 2^-60 of the sum.  The ratio is the derivative of the series:
    I_{nu+1} / I_nu = (2 / x) sum_k k t_k / sum_k t_k."""
    nu, x = float(nu), float(x)
    q = 0.25 * x * x
    k0 = math.floor(2.0 * q / (nu + math.sqrt(nu * nu + x * x)))
    log_t0 = k0 * math.log(q) - math.lgamma(k0 + 1.0) - math.lgamma(nu + k0 + 1.0)
    tiny = 2.0 ** -60
    s, sk, t = 1.0, float(k0), 1.0
    terms = 1
    for n in range(1, 1 << 14):
        k = k0 + float(n)
        t = t * (q / (k * (nu + k)))
        s += t
        sk += t * k
        terms += 1
        if t < tiny * s:
            break
    t = 1.0
    for n in range(1, 1 << 14):
        k = k0 - float(n)
        if k < 0.0:
            break
        t = t * (((k + 1.0) * (nu + k + 1.0)) / q)
        s += t
        sk += t * k
        terms += 1
        if t < tiny * s:
            break
    bessel.terms = terms
    return nu * math.log(0.5 * x) + log_t0 + math.log(s), (2.0 / x) * (sk / s)


def log_z(d, kappa):
    """-> (log Z_d(kappa), A_d(kappa)) in float64"""
    nu = 0.5 * d - 1.0
    li, a = bessel(nu, kappa)
    return nu * math.log(kappa) - (nu + 1.0) * LOG_2PI - li, a


def partition(theta, d):
    """theta [C] float32 -> dict: kappa [C] float32, logz [C] float64, logz32 [C] float32, ratio [C] float64, clamped [C] bool"""
    theta = np.asarray(theta, np.float32)
    with np.errstate(invalid='ignore'):
        inside = (theta >= THETA_LO) & (theta <= THETA_HI)
    tc = np.where(np.isnan(theta), THETA_LO, np.clip(theta, THETA_LO, THETA_HI)).astype(np.float32)
    kappa = np.exp(tc.astype(np.float64)).astype(np.float32)
    return dict(from_kappa(kappa, d), clamped=~inside)


def from_kappa(kappa, d):
    """the table at given float32 concentrations"""
    kappa = np.asarray(kappa, np.float32)
    lz = np.array([log_z(d, float(k)) for k in kappa], np.float64).reshape(-1, 2)
    return {'kappa': kappa, 'logz': lz[:, 0].copy(), 'logz32': lz[:, 0].astype(np.float32), 'ratio': lz[:, 1].copy()}


def row_sum(t):
    """[n, D] -> [n]: the sum in the product's order, in the dtype of t.  Lane j of 64 adds its elements j, j + 64, ... ascending; the
    lanes are then added by the xor tree 32, 16, ... 1."""
    n, D = t.shape
    nc = -(-D // 64)
    pad = np.zeros((n, nc * 64), t.dtype)
    pad[:, :D] = t
    pad = pad.reshape(n, nc, 64)
    v = np.zeros((n, 64), t.dtype)
    for k in range(nc):
        v = v + pad[:, k]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ o]
    return v[:, 0]


def unit(u):
    """rows u [n, d] -> (n = max(|u|, EPS) [n], u / n), in the dtype of u"""
    n = np.maximum(np.sqrt(row_sum(u * u)), u.dtype.type(EPS))
    return n, u / n[:, None]


def seq_dot(r, mu):
    """r [n, d], mu [C, d] -> [n, C]: acc = acc + mu_k * r_k for k = 0 .. d - 1 in order, in the dtype of r"""
    acc = np.zeros((r.shape[0], mu.shape[0]), r.dtype)
    for k in range(r.shape[1]):
        acc = acc + mu[None, :, k] * r[:, k, None]
    return acc


def flags(U, labels, A, C, valid=None):
    """-> [B * K] int: the label of an entry that counts, -1 not counted, -2 a non-finite row, -3 its class is not valid"""
    U = np.asarray(U, np.float32)
    B, P, d = U.shape
    lab = np.asarray(labels).reshape(B, -1)
    K = lab.shape[1]
    assert K == A * P
    if lab.dtype.kind == 'f':
        with np.errstate(invalid='ignore'):
            ok = (lab >= -2147483648.0) & (lab < 2147483648.0)
        lab = np.where(ok, np.where(ok, lab, 0).astype(np.int64), -1)          # (truncation, as the device converts)
    lab = lab.astype(np.int64).reshape(-1)
    out = np.where((lab >= 0) & (lab < C), lab, -1)
    if valid is not None:
        out = np.where((out >= 0) & ~np.asarray(valid, bool)[np.maximum(out, 0)], -3, out)
    fin = np.isfinite(U).all(2).reshape(-1)[np.arange(B * K) // A]
    return np.where((out >= 0) & ~fin, -2, out)


def update(U, labels, A, proto, valid, alpha=0.95, limit=None):
    """The ordered prototype update in float32 -> (prototypes [C, d] float32, valid [C] bool); the inputs are not changed."""
    U = np.asarray(U, np.float32)
    B, P, d = U.shape
    proto, valid = np.array(proto, np.float32), np.array(valid, bool)
    C = proto.shape[0]
    lab = flags(U, labels, A, C)
    rows = U.reshape(B * P, d)
    al, be = np.float32(alpha), np.float32(1.0) - np.float32(alpha)
    for c in range(C):
        idx = np.nonzero(lab == c)[0]
        if limit:
            idx = idx[:limit]
        if not len(idx):
            continue
        r = unit(rows[idx // A])[1]
        mu = proto[c]
        for i in range(len(idx)):
            mu = unit((al * mu + be * r[i])[None])[1][0]
        proto[c], valid[c] = mu, True
    return proto, valid


def update_literal(U, labels, A, proto, valid, alpha=0.95, limit=None):
    """The per-sample loop as the paper's code runs it: every counted sample in (b, j) order updates the prototype of its class."""
    U = np.asarray(U, np.float32)
    B, P, d = U.shape
    proto, valid = np.array(proto, np.float32), np.array(valid, bool)
    lab = flags(U, labels, A, proto.shape[0])
    taken = np.zeros(proto.shape[0], np.int64)
    al, be = np.float32(alpha), np.float32(1.0) - np.float32(alpha)
    for i in range(lab.shape[0]):
        c = lab[i]
        if c < 0 or (limit and taken[c] >= limit):
            continue
        u = U.reshape(B * P, d)[i // A][None]
        r = u / np.maximum(np.sqrt(row_sum(u * u)), np.float32(EPS))
        v = al * proto[c][None] + be * r
        proto[c] = (v / np.maximum(np.sqrt(row_sum(v * v)), np.float32(EPS)))[0]
        valid[c] = True
        taken[c] += 1
    return proto, valid


def logits(r, proto, valid, part):
    """unit rows r [n, d] (float32 or float64) -> (l [n, C] with -inf for a class that is not valid, dot [n, C])"""
    dt = r.dtype
    dot = seq_dot(r, np.asarray(proto, np.float32).astype(dt))
    l = part['logz32'].astype(dt)[None] + part['kappa'].astype(dt)[None] * dot
    l[:, ~np.asarray(valid, bool)] = -np.inf
    return l, dot


def forward(U, labels, A, proto, valid, part, dtype=np.float64):
    """-> dict: loss, dU [B, P, d], dtheta [C], m, skipped, valid_classes, mean_dot, mean_kappa, max_kappa and per counted row
    loss_i, dot_y, idx (entry), y.  With float32 the loss, dU and dtheta are rounded to float32 as the product stores them."""
    U = np.asarray(U, np.float32)
    B, P, d = U.shape
    valid = np.asarray(valid, bool)
    C = valid.shape[0]
    lab = flags(U, labels, A, C, valid)
    idx = np.nonzero(lab >= 0)[0]
    m, y, cell = len(idx), lab[idx], idx // A
    n, r = unit(U.reshape(B * P, d)[cell].astype(dtype))
    mu = np.asarray(proto, np.float32).astype(dtype)
    kap = part['kappa'].astype(dtype)
    out = {'m': m, 'skipped': int((lab == -2).sum()), 'valid_classes': int(valid.sum()), 'idx': idx, 'y': y,
           'mean_kappa': float(part['kappa'].astype(np.float64).mean()), 'max_kappa': float(part['kappa'].max())}
    dU = np.zeros((B * P, d), dtype)
    dtheta = np.zeros(C, np.float64)
    loss_i, dot_y = np.zeros(0, dtype), np.zeros(0, dtype)
    if m:
        with np.errstate(invalid='ignore'):
            l, dot = logits(r, proto, valid, part)
            mx = l.max(1)
            e = np.where(valid[None], np.exp(l - mx[:, None]), dtype(0))
            s = row_sum(e)
            lse = mx + np.log(s)
            p = e / s[:, None]
            rows = np.arange(m)
            loss_i, dot_y = lse - l[rows, y], dot[rows, y]
            hot = np.zeros((m, C), dtype)
            hot[rows, y] = 1
            g = np.where(valid[None], (p - hot) * dtype(1.0 / max(m, 1)), dtype(0))
            term = g.astype(np.float64) * (np.where(valid[None], dot, 0).astype(np.float64) - part['ratio'][None])
            dtheta = part['kappa'].astype(np.float64) * np.where(valid[None], term, 0.0).sum(0)
            w = g * kap[None]
            G = np.zeros((m, d), dtype)
            for c in range(C):
                G = G + w[:, c, None] * mu[c][None]
            gr = row_sum(G * r)
            du = (G - gr[:, None] * r) / n[:, None]
        for i in range(m):                                       # the counted anchors of a cell, ascending
            dU[cell[i]] = dU[cell[i]] + du[i]
    if 'clamped' in part:
        dtheta = np.where(part['clamped'], 0.0, dtheta)
    loss = float(loss_i.astype(np.float64).sum()) / max(m, 1)
    out.update(loss_i=loss_i, dot_y=dot_y, mean_dot=float(dot_y.astype(np.float64).sum()) / max(m, 1))
    if dtype == np.float32:
        loss, dtheta = np.float32(loss), dtheta.astype(np.float32)
    out.update(loss=loss, dU=dU.reshape(B, P, d), dtheta=dtheta)
    return out


def score(rows, proto, valid, part, dtype=np.float64):
    """rows [n, d] float32 -> dict vmf [n], vmf_class [n] int64, vmf_cosine [n], margin [n] (best minus second best logit) in `dtype`;
    0, -1, 0 without a valid class"""
    valid = np.asarray(valid, bool)
    rows = np.asarray(rows, np.float32).astype(dtype)
    nrow = rows.shape[0]
    if not valid.any():
        return {'vmf': np.zeros(nrow, dtype), 'vmf_class': np.full(nrow, -1, np.int64), 'vmf_cosine': np.zeros(nrow, dtype),
                'margin': np.full(nrow, np.inf), 'unit': unit(rows)[1]}
    r = unit(rows)[1]
    l, dot = logits(r, proto, valid, part)
    srt = np.sort(l, 1)
    margin = srt[:, -1] - srt[:, -2] if l.shape[1] > 1 else np.full(nrow, np.inf)
    return {'vmf': l.max(1), 'vmf_class': l.argmax(1).astype(np.int64), 'vmf_cosine': np.where(valid[None], dot, -np.inf).max(1),
            'margin': margin, 'unit': r}


def bound(ref, f32):
    """arrays (or scalars) of the float64 and the float32 restatement -> (E32, 4 E32 + 1e-7 max |value|); an empty array: (0, 0)"""
    ref, f32 = np.atleast_1d(np.asarray(ref, np.float64)), np.atleast_1d(np.asarray(f32, np.float64))
    if ref.size == 0:
        return 0.0, 0.0
    e32 = float(np.abs(f32 - ref).max())
    return e32, 4.0 * e32 + 1e-7 * float(np.abs(ref).max())


def bounds(ref, f32):
    """key -> (E32, bound) for dU and dtheta; for the loss and mean_dot the bound of the per-row loss_i / dot_y (a float64 mean of
    terms each within a bound is within it)"""
    return {'dU': bound(ref['dU'], f32['dU']), 'dtheta': bound(ref['dtheta'], f32['dtheta']),
            'loss': bound(ref['loss_i'], f32['loss_i']), 'mean_dot': bound(ref['dot_y'], f32['dot_y'])}


def inputs(B, P, d, A, C, n_counted, seed=0, spread=0.35):
    """A seeded embedding U [B, P, d] float32 (class directions plus noise) and dense labels [B, A P] int64 with exactly n_counted
    labels in [0, C) on the cells of their class, the rest drawn from (-1, -2, C, C + 5)."""
    rs = np.random.RandomState(9000 + 131 * d + 17 * C + n_counted + seed)
    K = A * P
    dirs = rs.normal(size=(C, d))
    cell_cls = rs.randint(0, C, (B, P))
    U = (dirs[cell_cls] + spread * math.sqrt(d) * rs.normal(size=(B, P, d))) * rs.uniform(0.5, 3.0, (B, P, 1))
    labels = rs.choice(np.array([-1, -2, C, C + 5], np.int64), size=(B, K), p=[0.7, 0.1, 0.1, 0.1])
    assert n_counted <= B * K
    pick = rs.choice(B * K, n_counted, replace=False)
    labels.reshape(-1)[pick] = cell_cls.reshape(-1)[pick // A]
    return U.astype(np.float32), labels
