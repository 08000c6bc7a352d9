"""ood_synth without a GPU: the numpy restatement of tests/_outlier_synth_ref.py against Philox's known answers, the moments of the
normals, the density identity that lets the selection work on |eps|^2 alone, scipy's Gaussian log-density, the subset rule, and the
argument checks of `OutlierSynthesizer` that need no device."""
import re

import numpy as np
import pytest

import _outlier_synth_ref as R

KNOWN = [
    ((0, 0, 0, 0), (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), 'd16cfe09 94fdcceb 5001e420 24126ea1'),
]


@pytest.mark.parametrize('ctr,key,want', KNOWN)
def test_philox_known_answers(ctr, key, want):
    got = R.philox(*[np.array([v]) for v in ctr], *key)
    assert ' '.join('%08x' % int(v[0]) for v in got) == want


def test_counter_layout():
    """candidate j, class c, block q, draw t and the seed sit where the kernel puts them"""
    seed, t, c, F = 0x0123456789abcdef, (5 << 32) | 7, 11, 12
    w = R.words(seed, t, c, np.array([3, 9]), F)
    for row, j in enumerate((3, 9)):
        for q in range(F // 4):
            got = R.philox(np.array([j]), np.array([c | q << 16]), np.array([7]), np.array([5]), 0x89abcdef, 0x01234567)
            assert [int(v[0]) for v in got] == [int(v) for v in w[row, 4 * q:4 * q + 4]]


@pytest.mark.parametrize('F', [64, 88, 288])
def test_distribution(F):
    S = 4000
    z64, z32 = R.candidates(3, 0, [5], S, F)
    z = z64[0]
    n = z.size
    assert np.isfinite(z).all() and np.isfinite(z32).all()
    assert abs(z.mean()) < 5.0 / np.sqrt(n)                                   # five standard errors of the mean
    assert abs(z.var() - 1.0) < 5.0 * np.sqrt(2.0 / n)
    r2 = R.sqnorm(z)
    assert abs(r2.mean() - F) < 5.0 * np.sqrt(2.0 * F / S)                    # chi^2_F: mean F, variance 2 F
    assert abs(np.corrcoef(z[:, 0], z[:, 1])[0, 1]) < 5.0 / np.sqrt(S)        # the cos and sin halves of a pair
    e32 = np.abs(R.sqnorm(z32[0]).astype(np.float64) - r2).max()
    print('F %d: E32 of r2 %.3g' % (F, e32))
    assert e32 < 1e-3


@pytest.mark.parametrize('F', [64, 88])
def test_density_identity(F):
    """(x - mu)^T Sigma^-1 (x - mu) = |eps|^2 for x = mu + L eps: the least likely candidate is the one with the largest norm"""
    mu, L = R.gaussians(F, 3, seed=F)
    z = R.candidates(1, 2, [2], 200, F)[0][0]
    x = R.rows(mu[2], L, z)
    d = x - mu[2]
    maha = np.einsum('nd,nd->n', d, np.linalg.solve(L @ L.T, d.T).T)
    r2 = R.sqnorm(z)
    assert np.abs(maha - r2).max() <= 1e-9 * r2.max()


def test_selection_against_scipy():
    from scipy.stats import multivariate_normal
    F, C, S, k = 64, 3, 500, 8
    mu, L = R.gaussians(F, C, seed=7)
    out = R.sample(11, 4, range(C), S, F, k, mu, L)
    # r2 descending = the least likely first, so log_density = -r2 / 2 + const runs the other way
    assert (np.diff(out['r2'], axis=1) <= 0).all() and (np.diff(out['log_density'], axis=1) >= 0).all()
    for c in range(C):
        want = multivariate_normal(mu[c], L @ L.T).logpdf(out['rows'][c])
        assert np.abs(want - out['log_density'][c]).max() < 1e-9 * np.abs(want).max()
        assert (out['r2'][c][-1] >= np.delete(out['r2_all'][c], out['index'][c])).all()      # nothing left out is less likely
    assert len(set(map(tuple, out['index']))) == C                                          # the classes draw different candidates


def test_selection_breaks_ties_by_the_smaller_index():
    r2 = np.array([1.0, 3.0, 2.0, 3.0, 0.5, 2.0], np.float32)
    assert R.select(r2, 6).tolist() == [1, 3, 2, 5, 0, 4]
    assert R.select(r2, 1).tolist() == [1]


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_subset_rule(dtype):
    F, C, S, k = 64, 6, 130, 3
    mu, L = R.gaussians(F, C, seed=3)
    valid = np.array([1, 1, 0, 1, 1, 1], bool)
    full = R.sample(5, 9, range(C), S, F, k, mu, L, valid, dtype)
    part = R.sample(5, 9, [4, 1, 2], S, F, k, mu, L, valid, dtype)
    for ci, c in enumerate([4, 1, 2]):
        for key in ('rows', 'index', 'r2', 'log_density'):
            assert np.array_equal(part[key][ci], full[key][c]), key
        assert np.array_equal(part['roles'][ci * k:(ci + 1) * k], full['roles'][c * k:(c + 1) * k])
    assert (full['rows'][2] == 0).all() and (full['roles'][2 * k:3 * k] == -1).all() and (np.delete(full['roles'], [6, 7, 8]) == 0).all()
    other = R.sample(5, 10, range(C), S, F, k, mu, L, valid, dtype)
    assert not np.array_equal(other['index'], full['index'])                                 # the next draw is another one


def test_float32_rows_follow_the_float64_ones():
    F = 88
    mu, L = R.gaussians(F, 2, seed=1)
    z64, z32 = R.candidates(2, 0, [1], 50, F)
    a, b = R.rows(mu[1], L, z64[0]), R.rows(mu[1], L, z32[0])
    assert b.dtype == np.float32 and np.abs(a - b).max() < 1e-4
    mu, I = R.gaussians(F, 2, seed=1, identity=True)
    assert np.array_equal(R.rows(np.zeros(F), I, z32[0]), z32[0])                            # L = I, mu = 0: the normals themselves
    assert np.array_equal(R.rows(mu[0], I, z32[0]), mu[0].astype(np.float32)[None] + z32[0])


def test_gaussian_factors():
    from ood_object_detection_amd.ood_synth import gaussian_factors
    g = np.random.default_rng(0)
    F, C = 8, 3
    cls = g.integers(0, 2, 400)                                                              # class 2 stays empty
    x = g.standard_normal((400, F)) @ g.standard_normal((F, F)) + cls[:, None]
    n_c = np.bincount(cls, minlength=C)
    s_c = np.stack([x[cls == c].sum(0) for c in range(C)])
    p = gaussian_factors(n_c, s_c, x.T @ x, min_count=5)
    assert p['valid'].tolist() == [True, True, False]
    assert np.allclose(p['L'] @ p['L'].T, p['cov']) and not np.triu(p['L'], 1).any()
    assert abs(p['log_const'] - R.log_const(p['L'])) < 1e-12
    with pytest.raises(ValueError):
        gaussian_factors(np.zeros(C, np.int64), np.zeros((C, F)), np.zeros((F, F)))
    with pytest.raises(ValueError):
        gaussian_factors(np.array([2, 1, 0]), s_c, x.T @ x)                                  # fewer rows than F: singular


def test_argument_checks():
    from ood_object_detection_amd.ood_synth import OutlierSynthesizer
    ok = dict(num_features=64, num_classes=90, num_anchors=9)
    for bad in (dict(num_features=60), dict(num_classes=0), dict(num_classes=1025), dict(num_anchors=0), dict(candidates=0),
                dict(candidates=(1 << 20) + 1), dict(num_classes=1024, candidates=1 << 17), dict(keep=0), dict(keep=10001),
                dict(min_count=0), dict(seed=-1), dict(seed=1 << 64), dict(statistics=object())):
        with pytest.raises(ValueError):
            OutlierSynthesizer(**{**ok, **bad})
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        OutlierSynthesizer(**ok, device='cpu')
    s = OutlierSynthesizer(**ok, keep=16, seed=(1 << 64) - 1)
    assert (s.S, s.k, s.fitted) == (10000, 16, False)
    with pytest.raises(RuntimeError, match='fit'):
        s.sample()
    for bad in ((np.zeros((90, 64)), np.eye(63)), (np.zeros((90, 64)), np.triu(np.ones((64, 64)))), (np.zeros((90, 64)), -np.eye(64)),
                (np.full((90, 64), np.nan), np.eye(64))):
        with pytest.raises(ValueError):
            s.set_gaussians(*bad)


def test_abi_is_declared_exported_and_bound():
    import os
    from ood_object_detection_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'effdet_hip.h')).read()
    names = sorted(n for n in _lib.SIGNATURES if n.startswith('effdet_outlier_synth'))
    assert names == ['effdet_outlier_synth', 'effdet_outlier_synth_workspace_bytes']
    for name in names:
        m = re.search(r'\b%s\(([^;]*)\);' % name, header)
        assert m, name
        assert len(_lib.SIGNATURES[name][1]) == m.group(1).count(',') + 1, name
    mk = open(os.path.join(root, 'ood_object_detection_amd', 'csrc', 'Makefile')).read()
    assert 'build/outlier_synth.o' in mk and 'EXTRA_outlier_synth = -ffp-contract=off' in mk
