"""Host-side checks of the feature-space OOD scores (ood_features.py, csrc/feature_ood.hip): the numpy restatement of
tests/_feature_ood_ref.py against scipy / scikit-learn, the raw-moment covariance against the centred form, the anchor -> cell
-> level addressing against `Anchors`, the C ABI and every refusal that needs no GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _feature_ood_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(F=64, C=7, n=1500, m=40):
    d = R.inputs(F, C, n, m)
    return d, R.finalize(*R.fit(d['x_fit'], d['y_fit'], C))


def test_restatement_against_scipy_and_sklearn():
    from scipy.spatial.distance import mahalanobis
    from sklearn.covariance import EmpiricalCovariance
    F, C = 64, 7
    d, p = _case(F, C)
    x, y = d['x_fit'].astype(np.float64), d['y_fit']
    # the tied covariance = the empirical covariance of the class-centred rows; the pooled Gaussian = that of the rows
    tied = EmpiricalCovariance(assume_centered=True).fit(x - p['mu'][y])
    pooled = EmpiricalCovariance().fit(x)
    assert np.abs(tied.covariance_ - p['cov']).max() <= 1e-9 * np.abs(p['cov']).max()
    assert np.abs(pooled.covariance_ - p['cov0']).max() <= 1e-9 * np.abs(p['cov0']).max()
    assert np.abs(pooled.location_ - p['mu0']).max() <= 1e-9 * np.abs(p['mu0']).max()
    s = R.score(d['x_in'], p)
    vi, vi0 = np.linalg.inv(tied.covariance_), np.linalg.inv(pooled.covariance_)
    xs = d['x_in'].astype(np.float64)
    worst = worst0 = 0.0
    for i in range(xs.shape[0]):
        for c in range(C):
            ref = mahalanobis(xs[i], p['mu'][c], vi) ** 2
            worst = max(worst, abs(s['d'][i, c] - ref) / ref)
        ref0 = mahalanobis(xs[i], pooled.location_, vi0) ** 2
        worst0 = max(worst0, abs(s['d0'][i] - ref0) / ref0)
    print('restatement against scipy: per-class distances %.2e, pooled %.2e (relative)' % (worst, worst0))
    assert worst <= 1e-9 and worst0 <= 1e-9
    # sklearn's own Mahalanobis of the pooled Gaussian
    assert np.abs(pooled.mahalanobis(xs) - s['d0']).max() <= 1e-9 * s['d0'].max()
    assert np.array_equal(s['nearest'], s['d'].argmin(1)) and np.allclose(s['relative'], -(s['d'].min(1) - s['d0']))


def test_raw_moment_covariance_against_the_centred_form():
    F, C = 88, 17
    d, p = _case(F, C, n=3000)
    x, y = d['x_fit'].astype(np.float64), d['y_fit']
    xc = x - p['mu'][y]
    cov = xc.T @ xc / x.shape[0]
    x0 = x - x.mean(0)
    cov0 = x0.T @ x0 / x.shape[0]
    e, e0 = np.abs(cov - p['cov']).max() / np.abs(cov).max(), np.abs(cov0 - p['cov0']).max() / np.abs(cov0).max()
    print('raw-moment against two-pass covariance: tied %.2e, pooled %.2e (relative to the largest entry)' % (e, e0))
    assert e <= 1e-10 and e0 <= 1e-10


def test_product_finalize_is_the_restatement():
    from ood_object_detection_amd import ood_features as of
    for shrink in (0.0, 0.05):
        d = R.inputs(112, 17, 2000, 10)
        st = R.fit(d['x_fit'], d['y_fit'], 17)
        a, b = of.finalize(*st, shrinkage=shrink), R.finalize(*st, shrinkage=shrink)
        for k in ('mu', 'mu0', 'cov', 'cov0', 'W', 'W0', 'M', 'm2'):
            assert np.abs(a[k] - b[k]).max() <= 1e-9 * np.abs(b[k]).max(), (k, shrink)
    # a class without rows: +inf, never the minimum
    st = R.fit(d['x_fit'], np.where(d['y_fit'] == 3, 4, d['y_fit']), 17)
    a = of.finalize(*st)
    assert a['m2'][3] == np.inf and np.isfinite(np.delete(a['m2'], 3)).all() and not a['M'][3].any()


@pytest.mark.parametrize('size', [128, 640])
def test_anchor_to_cell_to_level_against_anchors(size):
    from ood_object_detection_amd import ood_features as of
    from ood_object_detection_amd.effdet.anchors import Anchors
    anchors = Anchors(3, 7, 3, [1.0, 2.0, 0.5], 4.0, (size, size))
    A = anchors.get_anchors_per_location()
    boxes = anchors.boxes.numpy().astype(np.float64)
    hw = [tuple(anchors.feat_sizes[l]) for l in range(3, 8)]
    assert boxes.shape[0] == A * sum(h * w for h, w in hw)
    level, y, x = of.anchor_cells(np.arange(boxes.shape[0]), hw, A)
    stride = np.asarray([size // h for h, _ in hw], np.float64)[level]
    cy, cx = 0.5 * (boxes[:, 0] + boxes[:, 2]), 0.5 * (boxes[:, 1] + boxes[:, 3])
    assert np.abs(cy - (y + 0.5) * stride).max() <= 1e-3 and np.abs(cx - (x + 0.5) * stride).max() <= 1e-3
    assert level.min() == 0 and level.max() == 4 and (np.diff(level) >= 0).all()
    with pytest.raises(ValueError):
        of.anchor_cells([boxes.shape[0]], hw, A)


NAMES = ('effdet_feature_ood_workspace_bytes', 'effdet_feature_ood_fit', 'effdet_feature_ood_score')


def test_entry_points_declared_bound_and_exported():
    from ood_object_detection_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'effdet_hip.h')).read()
    lib = _lib.load()
    for name in NAMES:
        m = re.search(r'\b%s\s*\(([^;]*)\);' % name, header)
        assert m, name
        nargs = 0 if m.group(1).strip() == 'void' else m.group(1).count(',') + 1
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
        assert hasattr(lib, name), name
    mk = open(os.path.join(_lib.CSRC, 'Makefile')).read()
    assert 'build/feature_ood.o' in mk and re.search(r'EXTRA_feature_ood\s*=\s*-ffp-contract=off', mk)


def _table(n=1, cells=(100,), channel=1, F=64):
    lls = lambda v: (ctypes.c_longlong * len(v))(*v)
    buf = ctypes.create_string_buffer(64)
    base = ctypes.addressof(buf)
    return buf, (n, (ctypes.c_void_p * len(cells))(*[base] * len(cells)), lls(cells), lls([c * F for c in cells]), lls([F] * len(cells)),
                 lls([channel] * len(cells)))


def test_argument_refusals_before_any_launch():
    """every call below must return -22 from pure host code: this machine has no GPU to launch on"""
    from ood_object_detection_amd import _lib
    lib = _lib.load()
    q = lib.effdet_feature_ood_workspace_bytes
    assert 0 < q(1, 64) < q(100000, 64) < q(100000, 288) and q(1 << 27, 288) > 0
    for bad in ((0, 64), ((1 << 27) + 1, 64), (100, 96), (100, 0), (100, 384)):
        assert q(*bad) == -22, bad
    buf, ok = _table()
    p = ctypes.addressof(buf)                                 # any non-null address: nothing is dereferenced on the host

    def fit(table=ok, F=64, C=3, A=9, B=1, K=10, cdt=1, ws=1 << 30):
        return lib.effdet_feature_ood_fit(None, 0, *table, F, C, A, B, K, None, p, cdt, K, 1, 0, None, 0, p, p, p, p, ws)

    def score(table=ok, F=64, C=3, A=9, B=1, K=10, dtype=0):
        return lib.effdet_feature_ood_score(None, dtype, *table, F, C, A, B, K, None, None, 0, p, p, p, p, p, p, p, p)

    for fn in (fit, score):
        assert fn(F=96) == -22 and fn(F=0) == -22                                   # an unsupported width
        assert fn(C=0) == -22 and fn(C=1025) == -22                                 # classes out of range
        assert fn(table=_table(channel=2)[1]) == -22                                # a channel stride other than 1
        assert fn(table=_table(n=9, cells=(10,) * 9)[1]) == -22                     # more than 8 levels
        assert fn(table=_table(n=0)[1]) == -22 and fn(table=_table(cells=(0,))[1]) == -22
        assert fn(A=0) == -22 and fn(B=0) == -22 and fn(K=0) == -22 and fn(B=1 << 14, K=1 << 14) == -22
    assert score(dtype=2) == -22                                                    # float32 or bfloat16 features only
    assert fit(cdt=3) == -22 and fit(ws=64) == -22                                  # class dtype, a workspace too small


def test_python_refusals():
    from ood_object_detection_amd import ood_features as of
    with pytest.raises(ValueError, match='1024'):
        of.FeatureOOD(64, 1025, 9)
    with pytest.raises(ValueError):
        of.FeatureOOD(96, 3, 9)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        of.FeatureOOD(64, 3, 9, device='cpu')
    f = of.FeatureOOD(64, 3, 9)                               # nothing touches the device before the first add
    x = torch.zeros(2, 50, 64)
    with pytest.raises(RuntimeError, match='fit'):
        f.score(x, torch.zeros(2, 4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        f.add(x, torch.zeros(2, 450, dtype=torch.int64))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        f.add([torch.zeros(2, 64, 5, 5), torch.zeros(2, 64, 5, 5)], torch.zeros(2, 450, dtype=torch.int64))
    # a singular covariance: fewer rows than F, then exactly collinear rows; the message names the remedy
    d = R.inputs(64, 3, 40, 1)
    with pytest.raises(ValueError, match='shrinkage'):
        of.finalize(*R.fit(d['x_fit'], d['y_fit'], 3))
    of.finalize(*R.fit(d['x_fit'], d['y_fit'], 3), shrinkage=0.1)                   # ... which works
    d = R.inputs(64, 3, 500, 1)
    x = d['x_fit'].copy()
    x[:, 5] = x[:, 4]
    with pytest.raises(ValueError, match='more rows than F'):
        of.finalize(*R.fit(x, d['y_fit'], 3))
    with pytest.raises(ValueError, match='no rows'):
        of.finalize(np.zeros(3, np.int64), np.zeros((3, 64)), np.zeros((64, 64)))


def test_state_and_merge_on_the_numbers_alone():
    from ood_object_detection_amd import ood_features as of
    F, C = 64, 7
    d = R.inputs(F, C, 1200, 1)
    x, y = d['x_fit'], d['y_fit']

    def state(lo, hi):
        n_c, s_c, S = R.fit(x[lo:hi], y[lo:hi], C)
        return {'num_features': F, 'num_classes': C, 'num_anchors': 9, 'n_c': torch.from_numpy(n_c), 's_c': torch.from_numpy(s_c),
                'S': torch.from_numpy(S)}
    whole, merged = state(0, 1200), of.merged_state(state(0, 500), state(500, 1200))
    assert torch.equal(merged['n_c'], whole['n_c'])
    for k in ('s_c', 'S'):
        assert float((merged[k] - whole[k]).abs().max()) <= 1e-12 * float(whole[k].abs().max()), k
    a = of.finalize(merged['n_c'].numpy(), merged['s_c'].numpy(), merged['S'].numpy())
    b = of.finalize(whole['n_c'].numpy(), whole['s_c'].numpy(), whole['S'].numpy())
    assert np.abs(a['W'] - b['W']).max() <= 1e-9 * np.abs(b['W']).max()
    other = dict(state(0, 10), num_classes=8)
    with pytest.raises(ValueError):
        of.merged_state(whole, other)
