"""numpy restatement of ood_train.EnergyRegularizer (csrc/energy_reg.hip): the loss, its statistics and its analytic gradients.

`dtype=np.float64` is the reference.  `dtype=np.float32` is the yardstick: the same formulas in the product's operation order, the
per-row terms evaluated in float32 from the SAME float32 inputs (logits, temperature, margins, weights, phi rounded to float32) and
the sums over rows in float64, as the product adds them.  A row z of C logits has a role: 1 in-distribution, 0 outlier, anything
else does not count.

    logsumexp   mz = max z, m = mz / T, s = sum_k exp(z_k / T - m), E = -(T (m + log s)),   dE/dz_k = -(exp(z_k / T - m) / s)
    joint       E = -sum_k (max(z_k, 0) + log1p(exp(-|z_k|))),                              dE/dz_k = -(1 / (1 + exp(-z_k)))
    filter      an outlier row counts only when mz >= min_max_logit (numpy's max: a row that holds a NaN has a NaN maximum)
    hinge       in: d = E - m_in, out: d = m_out - E;  h = 0 where d < 0, else d;  l = h h,  dl/dE = +2 h (in), -2 h (out)
    logistic    sv = w (-E) + b;  in: l = softplus(-sv), dl/dsv = -sigmoid(-sv);  out: l = softplus(sv), dl/dsv = sigmoid(sv);
                dl/dE = dl/dsv (-w);  softplus(x) = max(x, 0) + log1p(exp(-|x|)), sigmoid(x) = 1 / (1 + exp(-x))
    loss        c_in sum_in l + c_out sum_out l,  c_side = weight_side / max(n_side, 1)  (float64)
    grad z_k    (c_side dl/dE) dE/dz_k  with c_side rounded to `dtype`;  zero in every row that does not count
    grad phi    (sum_side c_side sum dl/dsv (-E),  sum_side c_side sum dl/dsv)  (float64 sums; zero for the hinge)

The float32 form's distance from the reference, E32, measures what float32 arithmetic costs on the inputs at hand; the device is
held to 4 * E32 + 1e-7 * max |value| per key (`bound`)."""
import numpy as np

FORMS = ('hinge', 'logistic')
KINDS = ('logsumexp', 'joint')


def inputs(C, rows, seed=0):
    """logits 2 N(0, 1) - 3 rounded to float32, roles drawn from (1, 0, -1) (about 40 / 40 / 20 %), +5 on one random class of every
    in-distribution row -> z [rows, C] float32, role [rows] int8"""
    rs = np.random.RandomState(7000 + 31 * C + rows + seed)
    z = 2.0 * rs.normal(size=(rows, C)) - 3.0
    role = rs.choice(np.array([1, 0, -1], np.int8), size=rows, p=[0.4, 0.4, 0.2])
    hot = rs.randint(0, C, rows)
    z[np.arange(rows), hot] += np.where(role == 1, 5.0, 0.0)
    return z.astype(np.float32), role.astype(np.int8)


def widen_bf16(bits):
    """uint16 bfloat16 bits -> float32, exactly"""
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def _softplus(x):
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))


def _sigmoid(x):
    with np.errstate(over='ignore'):
        return 1 / (1 + np.exp(-x))


def row_sum(t):
    """[n, C] -> [n]: the sum over the classes in the product's order, in the dtype of t.  Lane j of 64 adds its classes j, j + 64, ...
    ascending; the lanes are then added by the xor tree 32, 16, ... 1 (after it every lane holds the same value)."""
    n, C = t.shape
    nc = -(-C // 64)
    pad = np.zeros((n, nc * 64), t.dtype)
    pad[:, :C] = t
    pad = pad.reshape(n, nc, 64)
    v = np.zeros((n, 64), t.dtype)
    for k in range(nc):
        v = v + pad[:, k]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ o]
    return v[:, 0]


def energy(z, kind='logsumexp', T=1.0, dtype=np.float64):
    """rows z [n, C] float32 -> E [n], dE/dz [n, C] in `dtype`"""
    zd = np.asarray(z, np.float32).astype(dtype)
    if kind == 'logsumexp':
        Td = dtype(np.float32(T))
        m = zd.max(1) / Td
        e = np.exp(zd / Td - m[:, None])
        s = row_sum(e)
        return -(Td * (m + np.log(s))), -(e / s[:, None])
    if kind != 'joint' or float(T) != 1.0:
        raise ValueError('kind / temperature')
    return -row_sum(_softplus(zd)), -_sigmoid(zd)


def sides(z, role, min_max=None):
    """-> [n] int: 0 the row does not count, 1 in-distribution, 2 outlier (after the filter on the exact float32 maximum)"""
    z, role = np.asarray(z, np.float32), np.asarray(role)
    side = np.where(role == 1, 1, np.where(role == 0, 2, 0))
    if min_max is not None:
        with np.errstate(invalid='ignore'):
            passes = z.max(1) >= np.float32(min_max)             # (False for a NaN maximum)
        side = np.where((side == 2) & ~passes, 0, side)
    return side


def forward(z, role, form, kind='logsumexp', T=1.0, m_in=None, m_out=None, w_in=1.0, w_out=1.0, min_max=None, phi=(1.0, 0.0),
            dtype=np.float64):
    """rows z [n, C] float32, role [n] -> dict: side, E, l, dE (dl/dE), dsv (dl/dsv), d (the hinge's argument) [n] (0 where the row does
    not count), energy (= E),
    loss, n_in, n_out, mean_l_in / out, mean_energy_in / out, active_in / out, grad_logits [n, C], grad_phi [2].  With float32 the
    loss, grad_logits and grad_phi are rounded to float32 as the product stores them; the means stay float64."""
    z = np.asarray(z, np.float32)
    n, C = z.shape
    side = sides(z, role, min_max)
    idx = np.nonzero(side)[0]
    sd = side[idx]
    out = {k: np.zeros(n, dtype) for k in ('E', 'l', 'dE', 'dsv', 'd')}
    gz = np.zeros((n, C), dtype)
    with np.errstate(invalid='ignore', over='ignore'):
        E, dEdz = energy(z[idx], kind, T, dtype)
        if form == 'hinge':
            d = np.where(sd == 1, E - dtype(np.float32(m_in)), dtype(np.float32(m_out)) - E)
            h = np.where(d < 0, dtype(0), d)
            l = h * h
            dE = np.where(sd == 1, 2 * h, -(2 * h))
            dsv = np.zeros_like(E)
            active = l > 0
            out['d'][idx] = d
        elif form == 'logistic':
            w, b = dtype(np.float32(phi[0])), dtype(np.float32(phi[1]))
            sv = w * (-E) + b
            l = np.where(sd == 1, _softplus(-sv), _softplus(sv))
            dsv = np.where(sd == 1, -_sigmoid(-sv), _sigmoid(sv))
            dE = dsv * (-w)
            active = np.zeros(len(idx), bool)
        else:
            raise ValueError('form')
        n_side = [int((sd == 1).sum()), int((sd == 2).sum())]
        c = [float(np.float32(w_in)) / max(n_side[0], 1), float(np.float32(w_out)) / max(n_side[1], 1)]
        l64, E64, dsv64 = l.astype(np.float64), E.astype(np.float64), dsv.astype(np.float64)
        tot = lambda v, s: float(v[sd == s].sum(dtype=np.float64))
        loss = c[0] * tot(l64, 1) + c[1] * tot(l64, 2)
        gphi = np.array([c[0] * tot(dsv64 * -E64, 1) + c[1] * tot(dsv64 * -E64, 2), c[0] * tot(dsv64, 1) + c[1] * tot(dsv64, 2)])
        cs = np.where(sd == 1, dtype(c[0]), dtype(c[1])).astype(dtype)
        gz[idx] = (cs * dE)[:, None] * dEdz
    out['E'][idx], out['l'][idx], out['dE'][idx], out['dsv'][idx] = E, l, dE, dsv
    out.update(side=side, form=form, energy=out['E'], n_in=n_side[0], n_out=n_side[1], active_in=int(active[sd == 1].sum()),
               active_out=int(active[sd == 2].sum()), mean_l_in=tot(l64, 1) / max(n_side[0], 1), mean_l_out=tot(l64, 2) / max(n_side[1], 1),
               mean_energy_in=tot(E64, 1) / max(n_side[0], 1), mean_energy_out=tot(E64, 2) / max(n_side[1], 1))
    if dtype == np.float32:
        loss, gphi = np.float32(loss), gphi.astype(np.float32)
    out.update(loss=loss, grad_logits=gz, grad_phi=gphi)
    return out


def bound(ref, f32):
    """arrays (or scalars) of the float64 and the float32 restatement -> (E32, 4 E32 + 1e-7 max |value|); an empty array: (0, 0)"""
    ref, f32 = np.atleast_1d(np.asarray(ref, np.float64)), np.atleast_1d(np.asarray(f32, np.float64))
    if ref.size == 0:
        return 0.0, 0.0
    e32 = float(np.abs(f32 - ref).max())
    return e32, 4.0 * e32 + 1e-7 * float(np.abs(ref).max())


def bounds(ref, f32, w_in=1.0, w_out=1.0):
    """key -> (E32, bound) for energy, grad_logits, grad_phi; for mean_l_side / mean_energy_side the bound of that side's per-row l /
    E (a float64 mean of terms each within a bound is within it); for the loss |w_in| bound(l in) + |w_out| bound(l out)."""
    out = {k: bound(ref[k], f32[k]) for k in ('energy', 'grad_logits', 'grad_phi')}
    for s, name in ((1, 'in'), (2, 'out')):
        rows = ref['side'] == s
        out['mean_l_' + name] = bound(ref['l'][rows], f32['l'][rows])
        out['mean_energy_' + name] = bound(ref['E'][rows], f32['E'][rows])
    out['loss'] = (abs(float(w_in)) * out['mean_l_in'][0] + abs(float(w_out)) * out['mean_l_out'][0],
                   abs(float(w_in)) * out['mean_l_in'][1] + abs(float(w_out)) * out['mean_l_out'][1])
    return out


def active_ranges(ref, tol):
    """The hinge's active counts that a float32 evaluation may report: side name -> (lowest, highest).  A row is active when its d > 0.
    The reference decides that for every row with |d| > tol (tol: the case's bound of the energy, of which d is an exact difference
    near zero); a row with |d| <= tol sits on the kink - a margin taken as the median of an odd number of energies puts exactly one row
    there, with d = 0 up to the rounding of the margin - and may be counted or not."""
    out = {}
    if ref['form'] != 'hinge':
        return {'in': (0, 0), 'out': (0, 0)}
    for s, name in ((1, 'in'), (2, 'out')):
        d = ref['d'][ref['side'] == s]
        sure = int((d > tol).sum())
        out[name] = (sure, sure + int((np.abs(d) <= tol).sum()))
    return out
