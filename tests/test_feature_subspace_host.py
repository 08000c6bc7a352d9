"""Host-side checks of the subspace OOD scores (ood_features.finalize_subspace / SubspaceFeatureOOD, csrc/feature_subspace.hip):
`finalize_subspace` against the projector form of the same scores, its choice of the principal dimension, its refusals and its
floor, the restatement of tests/_feature_subspace_ref.py under the eigen-solver's sign freedom, and the C ABI with every refusal
that needs no GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import _feature_subspace_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('effdet_feature_subspace_score', 'effdet_feature_subspace_calibrate', 'effdet_feature_subspace_workspace_bytes')


def _fs():
    from ood_object_detection_amd.ood_features import finalize_subspace
    return finalize_subspace


def _spectrum(lam, seed=0, n=1000):
    """(n_c, s_c, S) whose pooled covariance has exactly the eigenvalues lam (up to rounding) and a non-zero mean"""
    F = len(lam)
    rs = np.random.RandomState(seed)
    Q, _ = np.linalg.qr(rs.normal(size=(F, F)))
    cov = (Q * np.asarray(lam, np.float64)) @ Q.T
    mu = rs.normal(size=F)
    return np.array([n], np.int64), (n * mu)[None, :], n * (cov + np.outer(mu, mu)), Q, mu


@pytest.mark.parametrize('F', [64, 88])
def test_finalize_against_the_projector_form(F):
    d = R.inputs(F, 2048, 200)
    n_c, s_c, S = R.stats(d['x_fit'])
    x = d['x_ood'].astype(np.float64)
    mu0 = s_c[0] / n_c[0]
    cov0 = S / n_c[0] - np.outer(mu0, mu0)
    lam, U = np.linalg.eigh(0.5 * (cov0 + cov0.T))
    lam, U = lam[::-1], U[:, ::-1]
    xc = x - mu0
    for D in (0, 1, F // 2, F - 44, F - 1):
        p = _fs()(n_c, s_c, S, dim=D)
        assert p['dim'] == D and p['R'].shape == (F, F - D) and p['n'] == 2048 and p['inv_lambda'].shape == (F - D,)
        assert np.allclose(p['mu0'], mu0, rtol=0, atol=1e-14) and np.allclose(p['lambda'], lam, rtol=1e-10, atol=1e-14)
        y = (xc @ p['R'])
        r2 = (y * y).sum(1)
        proj = (xc * xc).sum(1) - ((xc @ U[:, :D]) ** 2).sum(1)
        assert np.abs(r2 - proj).max() <= 1e-10 * np.abs(proj).max(), D
        pm = (p['inv_lambda'][None, :] * y * y).sum(1)
        full = np.einsum('ni,ij,nj->n', xc, (p['R'] * p['inv_lambda'][None, :]) @ p['R'].T, xc)
        assert np.abs(pm - full).max() <= 1e-10 * np.abs(full).max(), D
        # independently: the pseudo-inverse of the covariance restricted to the trailing eigen-directions
        Pm = (U[:, D:] / lam[D:]) @ U[:, D:].T
        assert np.abs(pm - np.einsum('ni,ij,nj->n', xc, Pm, xc)).max() <= 1e-8 * np.abs(full).max(), D
    assert _fs()(n_c, s_c, S)['dim'] == F // 2                               # the default


def test_dimension_from_explained_variance():
    lam = np.array([8.0, 4.0, 2.0, 1.0, 0.5, 0.25, 0.125, 0.125])           # trace 16: the leading sums are 8, 12, 14, 15, 15.5, ...
    n_c, s_c, S, _, _ = _spectrum(lam)
    fs = _fs()
    for explained, D in ((0.4, 1), (0.5, 1), (0.51, 2), (0.75, 2), (0.76, 3), (0.875, 3), (0.9, 4), (0.95, 5), (0.999, 7), (1.0, 7)):
        assert fs(n_c, s_c, S, explained=explained)['dim'] == D, explained   # (capped at F - 1 = 7)
    for bad in (0.0, -0.1, 1.01, float('nan')):
        with pytest.raises(ValueError):
            fs(n_c, s_c, S, explained=bad)


def test_refusals_and_extreme_dimensions():
    F = 64
    d = R.inputs(F, 300, 10)
    n_c, s_c, S = R.stats(d['x_fit'])
    fs = _fs()
    with pytest.raises(ValueError, match='not both'):
        fs(n_c, s_c, S, dim=3, explained=0.9)
    for bad in (-1, F, F + 5, 2.5):
        with pytest.raises(ValueError):
            fs(n_c, s_c, S, dim=bad)
    with pytest.raises(ValueError, match='no rows'):
        fs(np.zeros(1, np.int64), np.zeros((1, F)), np.zeros((F, F)))
    p0, p1 = fs(n_c, s_c, S, dim=0), fs(n_c, s_c, S, dim=F - 1)
    assert p0['R'].shape == (F, F) and p1['R'].shape == (F, 1)
    assert np.allclose(p0['R'].T @ p0['R'], np.eye(F), atol=1e-12)          # D = 0: the residual is the whole centred feature
    x = d['x_ood'].astype(np.float64) - p0['mu0']
    assert np.allclose(((x @ p0['R']) ** 2).sum(1), (x * x).sum(1), rtol=1e-12)
    assert np.allclose(p1['R'][:, 0], p0['R'][:, -1]) or np.allclose(p1['R'][:, 0], -p0['R'][:, -1])
    # several classes pool into one mean
    two = fs(np.array([100, 200]), np.stack([d['x_fit'][:100].astype(np.float64).sum(0), d['x_fit'][100:].astype(np.float64).sum(0)]), S, dim=5)
    assert np.allclose(two['mu0'], fs(n_c, s_c, S, dim=5)['mu0'], rtol=0, atol=1e-13)


def test_floor_on_a_rank_deficient_matrix():
    F = 64
    rs = np.random.RandomState(3)
    x = rs.normal(size=(20, F))                                              # 20 rows: the covariance has rank <= 19
    n_c, s_c, S = R.stats(x)
    p = _fs()(n_c, s_c, S, dim=4, floor=1e-3)
    trace = p['lambda'].sum()
    low = 1e-3 * trace / F
    assert (p['lambda'][19:] < 1e-12 * trace).all() and np.isfinite(p['inv_lambda']).all()
    assert np.array_equal(p['inv_lambda'], 1.0 / np.maximum(p['lambda'][4:], low))
    assert np.allclose(p['inv_lambda'][19 - 4:], 1.0 / low, rtol=1e-12) and (p['inv_lambda'][:19 - 4] < 1.0 / low).all()
    with pytest.raises(ValueError):
        _fs()(n_c, s_c, S, floor=-1.0)


def test_scores_do_not_depend_on_the_eigenvector_signs():
    F = 88
    d = R.inputs(F, 1000, 100)
    p = _fs()(*R.stats(d['x_fit']), dim=44)
    flip = np.where(np.random.RandomState(5).uniform(size=44) < 0.5, -1.0, 1.0)
    q0 = R.params(p)
    q1 = R.params(dict(p, R=p['R'] * flip[None, :]))
    a = R.score(d['x_ood'], q0, logit=d['logit'][:100], alpha=0.5)
    b = R.score(d['x_ood'], q1, logit=d['logit'][:100], alpha=0.5)
    for k in R.KEYS:
        assert np.array_equal(a[k], b[k]), k                                 # y_i -> -y_i: every y_i^2 is the same number


def test_restatement_forms_agree():
    F = 64
    d = R.inputs(F, 1000, 100)
    q = R.params(_fs()(*R.stats(d['x_fit']), explained=0.9))
    ref = R.score(d['x_ood'], q, logit=d['logit'][:100], alpha=0.5)
    f32 = R.score(d['x_ood'], q, np.float32, logit=d['logit'][:100], alpha=0.5)
    assert all(f32[k].dtype == np.float32 for k in R.KEYS)
    for k, (e32, bound) in R.bounds(ref, f32).items():
        assert 0 < e32 <= 1e-5 * np.abs(ref[k]).max() and bound >= 4 * e32, k
    # vim: the float32 form rounds the product, then the difference; max_logit keeps the sign of the logit score
    assert np.array_equal(f32['vim'], -d['logit'][:100] - np.float32(0.5) * f32['r'])
    pos = R.score(d['x_ood'], q, np.float32, logit=d['logit'][:100], alpha=0.5, negate=False)
    assert np.array_equal(pos['vim'], d['logit'][:100] - np.float32(0.5) * f32['r'])
    # bfloat16 bits widen exactly
    bits = np.array([0x3F80, 0xC000, 0x0001, 0x7F7F], np.uint16)
    assert np.array_equal(R.widen_bf16(bits), np.array([1.0, -2.0, 2.0 ** -133, 3.3895313892515355e38], np.float32))


def test_entry_points_declared_bound_and_exported():
    from ood_object_detection_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'effdet_hip.h')).read()
    lib = _lib.load()
    for name in NAMES:
        m = re.search(r'\b%s\s*\(([^;]*)\);' % name, header)
        assert m, name
        assert len(_lib.SIGNATURES[name][1]) == m.group(1).count(',') + 1, name
        assert hasattr(lib, name), name
    mk = open(os.path.join(_lib.CSRC, 'Makefile')).read()
    assert 'build/feature_subspace.o' in mk and re.search(r'EXTRA_feature_subspace\s*=\s*-ffp-contract=off', mk)
    assert re.search(r'build/feature_subspace\.o:\s*feature_rows\.h', mk)
    src = open(os.path.join(_lib.CSRC, 'feature_subspace.hip')).read()
    assert '#include "feature_rows.h"' in src and 'fo_row(const FoLevels' not in src      # the row addressing is stated once
    assert re.search(r'build/feature_subspace\.o:\s*feature_rows\.h compact\.h', mk)
    assert 'fo_stage_centered<NT>(' in src and 'struct FsGeom' not in src and 'fs_stage' not in src     # ... and so are geometry and staging
    assert 'atomicAdd' not in src and 'mfma_f32_16x16x32_bf16' not in src                 # no atomics, no bf16 product


def _table(n=1, cells=(100,), channel=1, F=64):
    lls = lambda v: (ctypes.c_longlong * len(v))(*v)
    buf = ctypes.create_string_buffer(64)
    base = ctypes.addressof(buf)
    return buf, (n, (ctypes.c_void_p * len(cells))(*[base] * len(cells)), lls(cells), lls([c * F for c in cells]), lls([F] * len(cells)),
                 lls([channel] * len(cells)))


def test_argument_refusals_before_any_launch():
    """every call below must return -22 from pure host code: nothing is launched"""
    from ood_object_detection_amd import _lib
    lib = _lib.load()
    q = lib.effdet_feature_subspace_workspace_bytes
    assert 0 < q(1) <= q(100) < q(1 << 27)
    assert q(0) == -22 and q(-1) == -22 and q((1 << 27) + 1) == -22
    buf, ok = _table()
    p = ctypes.addressof(buf)                                 # any non-null address: nothing is dereferenced on the host

    def score(table=ok, dtype=0, F=64, A=9, B=1, K=10, Rp=32, Rt=p, il=p, mu0=p, ls=None, pitch=10, stride=1, res=p, pm=p, vim=None):
        return lib.effdet_feature_subspace_score(None, dtype, *table, F, A, B, K, None, None, 0, Rt, il, mu0, Rp, ls, pitch, stride, 1, 0.5,
                                                 res, pm, vim)

    def calibrate(table=ok, dtype=0, F=64, A=9, B=1, K=10, Rp=32, Rt=p, mu0=p, ls=p, pitch=10, stride=1, n=p, sums=p, ws=p, nbytes=1 << 30):
        return lib.effdet_feature_subspace_calibrate(None, dtype, *table, F, A, B, K, None, None, 0, Rt, mu0, Rp, ls, pitch, stride, 1, n, sums,
                                                     ws, nbytes)

    for fn in (score, calibrate):
        assert fn(F=96) == -22 and fn(F=0) == -22                                   # an unsupported width
        assert fn(table=_table(channel=2)[1]) == -22                                # a channel stride other than 1
        assert fn(table=_table(n=9, cells=(10,) * 9)[1]) == -22                     # more than 8 levels
        assert fn(table=_table(n=0)[1]) == -22 and fn(table=_table(cells=(0,))[1]) == -22
        assert fn(A=0) == -22 and fn(B=0) == -22 and fn(K=0) == -22 and fn(B=1 << 14, K=1 << 14) == -22
        assert fn(dtype=2) == -22                                                   # float32 or bfloat16 features only
        assert fn(Rp=0) == -22 and fn(Rp=-16) == -22 and fn(Rp=24) == -22 and fn(Rp=80) == -22      # 16 <= Rp <= Fp, a multiple of 16
        assert fn(Rt=None) == -22 and fn(mu0=None) == -22
        assert fn(ls=p, pitch=-1) == -22 and fn(ls=p, stride=-1) == -22
    assert score(il=None) == -22 and score(res=None) == -22 and score(pm=None) == -22
    assert score(vim=p) == -22                                                      # vim without a logit score
    assert calibrate(ls=None) == -22 and calibrate(n=None) == -22 and calibrate(sums=None) == -22 and calibrate(ws=None) == -22
    assert calibrate(nbytes=8) == -22                                               # a workspace too small


def test_scorer_list_refuses_a_key_collision():
    from ood_object_detection_amd.effdet.bench import _feature_scorers
    from ood_object_detection_amd.ood_features import FeatureOOD, SubspaceFeatureOOD
    m = FeatureOOD(64, 3, 9)                     # (constructors allocate nothing: no device is needed here)
    a, b = SubspaceFeatureOOD(64, 3, 9, statistics=m), SubspaceFeatureOOD(64, 3, 9, logit='max_logit')
    assert a.KEYS == ('residual', 'partial_mahalanobis', 'vim') and a.WANTS_LOGIT_SCORE is True
    assert a.statistics is m and b.statistics is not m and (b.F, b.C, b.A) == (64, 3, 9)
    assert _feature_scorers([m, a]) == (m, a) and _feature_scorers(a) == (a,)
    with pytest.raises(ValueError, match='residual'):
        _feature_scorers([a, m, b])
    with pytest.raises(ValueError, match='geometry'):
        SubspaceFeatureOOD(64, 4, 9, statistics=m)


def test_constructor_refusals_need_no_device():
    from ood_object_detection_amd.ood_features import SubspaceFeatureOOD
    with pytest.raises(ValueError, match='logit'):
        SubspaceFeatureOOD(64, 3, 9, logit='softmax')
    with pytest.raises(ValueError):
        SubspaceFeatureOOD(65, 3, 9)
    with pytest.raises(RuntimeError):
        SubspaceFeatureOOD(64, 3, 9, device='cpu')
    with pytest.raises(ValueError, match='statistics'):
        SubspaceFeatureOOD(64, 3, 9, statistics=object())
