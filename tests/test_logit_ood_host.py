"""Host-side checks of the logit-space OOD scores (ood_logits.finalize / LogitOOD, csrc/logit_ood.hip): the two precisions of the
restatement of tests/_logit_ood_ref.py against each other, its log-domain formulas against the literal ones in float64, the host
glue of `fit`, and the C ABI with every refusal that needs no GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import _logit_ood_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('effdet_logit_ood_score', 'effdet_logit_ood_fit', 'effdet_logit_ood_workspace_bytes')


def _finalize():
    from ood_object_detection_amd.ood_logits import finalize
    return finalize


def _case(C, T=1.0, top_m=10):
    d = R.inputs(C)
    q = R.params(_finalize()(*R.stats(d['z_fit'], C, T)))
    z = np.concatenate([d['z_in'], d['z_ood']])
    kw = dict(T=T, top_m=top_m, q=q)
    return z, R.score(z, **kw), R.score(z, np.float32, **kw)


@pytest.mark.parametrize('C,T,top_m', [(2, 1.0, 10), (7, 1.0, 10), (7, 2.5, 1), (90, 1.0, 10), (90, 2.5, 95)])
def test_restatement_forms_agree(C, T, top_m):
    z, ref, f32 = _case(C, T, top_m)
    assert all(f32[k].dtype == np.float32 for k in R.FLOAT_KEYS)
    for k, (e32, bound) in R.bounds(ref, f32).items():
        print('C %d T %.1f top_m %d %s: max |value| %.3g, E32 %.2e' % (C, T, top_m, k, np.abs(ref[k]).max(), e32))
        assert 0 < e32 <= 1e-5 * np.abs(ref[k]).max() and bound >= 4 * e32, k
    assert np.array_equal(ref['predicted_class'], f32['predicted_class'])
    sure = ref['kl_margin'] >= 2 * R.bounds(ref, f32)['kl_matching'][1]
    assert sure.all() and np.array_equal(ref['kl_class'][sure], f32['kl_class'][sure])       # the seeded draw excludes no row
    assert (ref['neg_entropy'] <= 0).all() and (ref['gen'] <= 0).all() and (ref['msp'] <= 1).all() and (ref['joint_energy'] >= 0).all()
    # bfloat16 bits widen exactly
    bits = np.array([0x3F80, 0xC000, 0x0001, 0x7F7F], np.uint16)
    assert np.array_equal(R.widen_bf16(bits), np.array([1.0, -2.0, 2.0 ** -133, 3.3895313892515355e38], np.float32))


@pytest.mark.parametrize('C,T,top_m', [(1, 1.0, 10), (2, 1.0, 10), (7, 2.5, 3), (90, 1.0, 10), (90, 1.0, 100)])
def test_formulas_against_their_literal_forms(C, T, top_m):
    d = R.inputs(C)
    z = np.concatenate([d['z_in'], d['z_ood']])
    ref = R.score(z, T=T, top_m=top_m)
    u = z.astype(np.float64) / T
    lse = np.log(np.exp(u - u.max(1, keepdims=True)).sum(1)) + u.max(1)
    p = np.exp(u - lse[:, None])
    m_ = min(top_m, C)
    top = -np.sort(-p, axis=1)[:, :m_]                                       # p is monotone in u
    gamma = float(np.float32(0.1))
    lit = -(top ** gamma * (1.0 - top) ** gamma).sum(1)
    assert np.abs(ref['gen'] - lit).max() <= 1e-9 * max(np.abs(lit).max(), 1e-300), np.abs(ref['gen'] - lit).max()
    if C == 1:
        assert (ref['gen'] == 0).all() and (ref['msp'] == 1).all() and (ref['neg_entropy'] == 0).all()
    energy = -lse
    assert np.abs(ref['msp'] - np.exp(u.max(1) + energy)).max() <= 1e-12
    assert np.abs(ref['neg_entropy'] - (p * np.log(np.maximum(p, 1e-300))).sum(1)).max() <= 1e-12 * max(np.abs(ref['neg_entropy']).max(), 1.0)
    zd = z.astype(np.float64)
    assert (zd < 700).all()
    je = np.log1p(np.exp(zd)).sum(1)
    assert np.abs(ref['joint_energy'] - je).max() <= 1e-12 * je.max()


def test_log_domain_gen_survives_an_extreme_row():
    z = np.full((1, 5), -100.0, np.float32)
    z[0, 0] = 88.0
    for dt in (np.float64, np.float32):
        out = R.score(z, dt, top_m=5)
        assert all(np.isfinite(out[k]).all() for k in ('msp', 'neg_entropy', 'gen', 'joint_energy')), dt
        assert out['predicted_class'][0] == 0 and out['msp'][0] == 1
    # exact ties: the lowest index is the predicted class, and the top_m cut takes the lower classes first
    t = np.array([[1.0, 3.0, 3.0, -2.0, 3.0]], np.float32)
    assert R.score(t)['predicted_class'][0] == 1
    one, two, three = (R.score(t, top_m=m)['gen'][0] for m in (1, 2, 3))
    assert one > two > three and abs((two - one) - (three - two)) <= 1e-12       # equal logits give equal terms


def test_fit_host_glue():
    fin = _finalize()
    C = 5
    rs = np.random.RandomState(1)
    n_c = np.array([40, 0, 1, 25, 0], np.int64)
    P = rs.dirichlet(np.ones(C), size=C) * n_c[:, None]
    mz = [rs.normal(2.0, 1.5, n) for n in n_c]
    a_c = np.array([v.sum() for v in mz])
    b_c = np.array([(v * v).sum() for v in mz])
    p = fin(n_c, P, a_c, b_c, smoothing=1e-3, std_floor=1e-3)
    have = n_c > 0
    assert np.array_equal(p['have'], have) and p['n'] == 66
    assert np.allclose(np.exp(p['log_d'][have]).sum(1), 1.0, rtol=0, atol=1e-12)       # smoothing keeps the rows normalised
    assert np.allclose(np.exp(p['log_d'][0]), (1 - 1e-3) * P[0] / 40 + 1e-3 / C, rtol=1e-13)
    assert not p['log_d'][~have].any() and np.array_equal(p['kl_inf'], np.where(have, 0.0, np.inf))
    # a class without rows gets +inf in the restatement, and is never the matching class
    z = (2.0 * rs.normal(size=(50, C))).astype(np.float32)
    out = R.score(z, q=R.params(p))
    assert np.isinf(out['kl'][:, ~have]).all() and np.isfinite(out['kl'][:, have]).all() and have[out['kl_class']].all()
    # moments: classes with at least two rows use their own, the others the pooled ones
    allz = np.concatenate(mz)
    for c in (0, 3):
        assert np.isclose(p['mu'][c], mz[c].mean(), rtol=1e-12) and np.isclose(p['sigma'][c], mz[c].std(), rtol=1e-10)
    for c in (1, 2, 4):
        assert np.isclose(p['mu'][c], allz.mean(), rtol=1e-12) and np.isclose(p['sigma'][c], allz.std(), rtol=1e-10)
    assert np.allclose(p['inv_sigma'], 1.0 / p['sigma'])
    # the floor
    q = fin(np.array([3, 0]), np.array([[2.0, 1.0], [0.0, 0.0]]), np.array([6.0, 0.0]), np.array([12.0, 0.0]), std_floor=0.25)
    assert (q['sigma'] == 0.25).all() and (q['inv_sigma'] == 4.0).all()
    # refusals
    with pytest.raises(ValueError, match='no rows'):
        fin(np.zeros(C, np.int64), np.zeros((C, C)), np.zeros(C), np.zeros(C))
    for bad in (0.0, -1e-6, 1.5, float('nan')):
        with pytest.raises(ValueError, match='smoothing'):
            fin(n_c, P, a_c, b_c, smoothing=bad)
    with pytest.raises(ValueError, match='std_floor'):
        fin(n_c, P, a_c, b_c, std_floor=0.0)


def test_entry_points_declared_bound_and_exported():
    from ood_object_detection_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'effdet_hip.h')).read()
    lib = _lib.load()
    for name in NAMES:
        m = re.search(r'\b%s\s*\(([^;]*)\);' % name, header)
        assert m, name
        assert len(_lib.SIGNATURES[name][1]) == m.group(1).count(',') + 1, name
        assert hasattr(lib, name), name
    assert sorted(n for n in _lib.SIGNATURES if n.startswith('effdet_logit_ood_')) == sorted(NAMES)
    mk = open(os.path.join(_lib.CSRC, 'Makefile')).read()
    assert 'build/logit_ood.o' in mk and re.search(r'EXTRA_logit_ood\s*=\s*-ffp-contract=off', mk)
    assert re.search(r'build/logit_ood\.o:\s*feature_rows\.h', mk)
    src = open(os.path.join(_lib.CSRC, 'logit_ood.hip')).read()
    assert '#include "feature_rows.h"' in src and 'fo_block_excl_scan(unsigned' not in src      # the compaction helpers are stated once
    assert re.search(r'build/logit_ood\.o:\s*feature_rows\.h compact\.h', mk)
    assert not re.search(r'void \w+_(count|base)_kernel\(', src) and 'fo_count_kernel<LoArgs>' in src      # ... and so are its launches
    assert 'atomicAdd' not in src and 'mfma_f32_16x16x32_bf16' not in src                       # no atomics, no bf16 product
    assert 'mma_chunk(' in src                                                                   # the float32-input MFMA of common.h


def test_wave_per_row_primitives_are_stated_once():
    """what the units that walk a row with one wave share is wave_rows.h's; none of them keeps a copy of its own"""
    from ood_object_detection_amd import _lib
    mk = open(os.path.join(_lib.CSRC, 'Makefile')).read()
    shared = open(os.path.join(_lib.CSRC, 'wave_rows.h')).read()
    assert '#include "compact.h"' in shared
    for text in ('DEV int wr_min(int', 'DEV unsigned wr_top(', 'DEV float wr_argmax(', 'DEV void wr_load(', 'DEV void wr_lse(',
                 'DEV float wr_softplus(float', 'void wr_for_classes(int'):
        assert shared.count(text) == 1, text
    for unit in ('logit_ood', 'act_shaping', 'energy_reg'):
        src = open(os.path.join(_lib.CSRC, unit + '.hip')).read()
        assert '#include "wave_rows.h"' in src, unit
        assert re.search(r'build/%s\.o:.*\bwave_rows\.h' % unit, mk), unit
        assert 'cand = tau |' not in src and 'key[i] >= cand' not in src, unit                 # the 32-step top-k search
        assert '__shfl_xor(v, o, 64); v = w < v' not in src and not re.search(r'DEV int \w+_min\(', src), unit     # the wave min
        assert 'log1pf(expf(-fabsf(' not in src and not re.search(r'\w+_softplus\(float', src), unit              # softplus
        assert not re.search(r'\bCp? <= 128\b', src) and 'wr_for_classes(' in src, unit          # the dispatch on the class count
        assert not re.search(r'int \w+_NONE\b', src), unit
        assert '_fit_write_kernel' not in src and 'const auto up' not in src, unit
    for unit in ('logit_ood', 'act_shaping'):
        src = open(os.path.join(_lib.CSRC, unit + '.hip')).read()
        assert 'wr_top<' in src and 'fo_write_index_kernel<' in src, unit
    assert open(os.path.join(_lib.CSRC, 'compact.h')).read().count('void fo_write_index_kernel(A a)') == 1
    assert 'const auto up' not in open(os.path.join(_lib.CSRC, 'outlier_synth.hip')).read()


def test_argument_refusals_before_any_launch():
    """every call below must return -22 from pure host code: nothing is launched"""
    from ood_object_detection_amd import _lib
    lib = _lib.load()
    q = lib.effdet_logit_ood_workspace_bytes
    assert 0 < q(1, 1) <= q(100, 90) < q(1 << 27, 90) and q(100, 90) < q(100, 1024)
    assert q(0, 90) == -22 and q(-1, 90) == -22 and q((1 << 27) + 1, 90) == -22 and q(100, 0) == -22 and q(100, 1025) == -22
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)                                 # any non-null address: nothing is dereferenced on the host

    def score(dtype=0, z=p, bs=900, as_=90, C=90, B=1, N=10, K=10, T=1.0, gamma=0.1, top_m=10, fitted=(None,) * 4, outs=(p,) * 5, kl=(None,) * 3):
        return lib.effdet_logit_ood_score(None, dtype, z, bs, as_, C, B, N, K, None, None, 0, T, gamma, top_m, *fitted, *outs, *kl)

    def fit(dtype=0, z=p, bs=900, as_=90, C=90, B=1, N=10, K=10, T=1.0, use_min=0, thr=0.0, stats=(p,) * 4, ws=p, nbytes=1 << 30):
        return lib.effdet_logit_ood_fit(None, dtype, z, bs, as_, C, B, N, K, None, None, 0, T, use_min, thr, *stats, ws, nbytes)

    for fn in (score, fit):
        assert fn(dtype=2) == -22 and fn(dtype=-1) == -22                          # float32 or bfloat16 logits only
        assert fn(z=None) == -22 and fn(bs=-1) == -22 and fn(as_=-1) == -22
        assert fn(C=0) == -22 and fn(C=1025) == -22
        assert fn(B=0) == -22 and fn(N=0) == -22 and fn(N=(1 << 31) + 1) == -22 and fn(K=0) == -22 and fn(B=1 << 14, K=1 << 14) == -22
        assert fn(T=0.0) == -22 and fn(T=-1.0) == -22 and fn(T=float('nan')) == -22 and fn(T=float('inf')) == -22
    assert score(gamma=float('nan')) == -22 and score(gamma=float('inf')) == -22 and score(top_m=0) == -22
    for k in range(5):
        assert score(outs=tuple(None if i == k else p for i in range(5))) == -22
    assert score(fitted=(p,) * 4) == -22 and score(kl=(p,) * 3) == -22             # the fitted parameters and their outputs come together
    assert score(fitted=(p, p, p, None), kl=(p,) * 3) == -22 and score(fitted=(p,) * 4, kl=(p, None, p)) == -22
    for k in range(4):
        assert fit(stats=tuple(None if i == k else p for i in range(4))) == -22
    assert fit(ws=None) == -22 and fit(nbytes=8) == -22 and fit(nbytes=q(10, 90) - 1) == -22
    assert fit(use_min=1, thr=float('nan')) == -22


def test_constructor_refusals_and_the_scorer_list():
    from ood_object_detection_amd.effdet.bench import _feature_scorers
    from ood_object_detection_amd.ood_features import FeatureOOD
    from ood_object_detection_amd.ood_logits import LogitOOD
    a = LogitOOD(3)                              # (constructors allocate nothing: no device is needed here)
    assert a.KEYS == R.KEYS and a.WANTS_CLASS_LOGITS is True and (a.temperature, a.gamma, a.top_m) == (1.0, 0.1, 10)
    m = FeatureOOD(64, 3, 9)
    assert _feature_scorers([m, a]) == (m, a) and _feature_scorers(a) == (a,)
    with pytest.raises(ValueError, match='msp'):
        _feature_scorers([a, m, LogitOOD(3, temperature=2.0)])
    for kw in (dict(num_classes=0), dict(num_classes=1025), dict(num_classes=3, temperature=0.0), dict(num_classes=3, temperature=float('nan')),
               dict(num_classes=3, gamma=float('inf')), dict(num_classes=3, top_m=0)):
        with pytest.raises(ValueError):
            LogitOOD(**kw)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        LogitOOD(3, device='cpu')
    import torch
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        a.score(torch.zeros(1, 4, 3), torch.zeros(1, 2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        a.add([torch.zeros(1, 9 * 3, 2, 2)])
