"""ood_features.SubspaceFeatureOOD (csrc/feature_subspace.hip) against the numpy restatement of tests/_feature_subspace_ref.py.

Inputs (`_feature_subspace_ref.inputs`): a fixed orthogonal Q, scales geomspace(1, 0.1, F) (covariance condition 100), a mean
1.5 N(0, 1) + 0.75, features mu + g A^T rounded to float32; 2048 fit rows (added on the device), 500 in-distribution and 500 "OOD"
rows (the same draw plus unit noise) to score, logit scores N(2, 3).

Bounds.  residual, partial_mahalanobis and vim: within 4 E32 + 1e-7 max |value| of the float64 restatement, per key; E32 is the
float32 restatement's own error on the same inputs, and both sides start from the SAME float32 Rt / inv_lambda / mu0 (the
device's `params` rounded as `fit` uploads them), so the eigen-solver's freedom is not part of the comparison.  Both terms come
from the restatement over the whole case of 1000 rows, never from the device; a test that scores a subset of those rows keeps the
case's bound (the E32 of a handful of rows is a noisy sample of the same quantity).  No row is excluded.  Every case prints E32
and the device error before it asserts.  Measured on an MI355X (device error / E32, worst key, per width at F - D = 1, the
non-multiple of 16, F): see the accuracy table of DESIGN.md §8."""
import numpy as np
import pytest
import torch

import _feature_subspace_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
WIDTHS = (64, 88, 112, 160, 224, 288)
ODD = {64: 44, 88: 44, 112: 44, 160: 100, 224: 100, 288: 100}            # an F - D that is no multiple of 16
ROW_COUNTS = (1, 15, 16, 17, 47, 48, 49, 63, 65)                        # around the 16-row wave and the 48- / 64-row workgroup
A, C = 3, 4
N_FIT, N_Q = 2048, 500
ALPHA = 0.75
_STATS, _CASES = {}, {}


def _place(x, B, seed=0, dtype=torch.float32):
    """n rows -> a [B, P, F] pyramid tensor that holds them at shuffled cells among other values, anchors [B, K] (cell * A +
    something) and count [B] (the last images hold the remainder, so count < K on some): row (b, j), j < count[b], is x[b * K + j]"""
    n, F = x.shape
    K = -(-n // B)
    P = K + 5
    rs = np.random.RandomState(n + 7 * B + seed)
    pyr = rs.normal(size=(B, P, F)).astype(np.float32)
    cell = np.stack([rs.permutation(P)[:K] for _ in range(B)])
    count = np.clip(n - K * np.arange(B), 0, K).astype(np.int32)
    xs = np.zeros((B * K, F), np.float32)
    xs[:n] = x
    live = np.arange(K)[None, :] < count[:, None]
    pyr[np.arange(B)[:, None].repeat(K, 1)[live], cell[live]] = xs.reshape(B, K, F)[live]
    anchor = cell * A + rs.randint(0, A, cell.shape)
    return torch.from_numpy(pyr).to(DEV).to(dtype), torch.from_numpy(anchor.astype(np.int64)).to(DEV), torch.from_numpy(count).to(DEV), live


def _logits(values, live):
    """[n] float32 -> a [B, K] device tensor with them on the live entries (777 elsewhere)"""
    out = np.full(live.shape, 777.0, np.float32)
    out[live] = values
    return torch.from_numpy(out).to(DEV)


def _statistics(F):
    """one FeatureOOD per width, filled once with the 2048 fit rows (two calls, classes 0 .. 3), left unchanged"""
    if F not in _STATS:
        from ood_object_detection_amd.ood_features import FeatureOOD
        d = R.inputs(F, N_FIT, N_Q)
        st = FeatureOOD(F, C, A, DEV)
        for part, B in ((d['x_fit'][:800], 3), (d['x_fit'][800:], 4)):
            lv, an, cnt, live = _place(part, B)
            cls = torch.from_numpy((np.arange(live.size).reshape(live.shape) % C).astype(np.int64)).to(DEV)
            st.add(lv, cls, an, cnt)
        torch.cuda.synchronize()
        assert int(st.n_c.sum()) == N_FIT
        _STATS[F] = (d, st)
    return _STATS[F]


def _case(F, Rn, logit='energy'):
    """the fitted scorer of (F, F - D = Rn), the restatement of its 1000 rows in both precisions and the bounds; left unchanged"""
    key = (F, Rn, logit)
    if key not in _CASES:
        from ood_object_detection_amd.ood_features import SubspaceFeatureOOD
        d, st = _statistics(F)
        f = SubspaceFeatureOOD(F, C, A, statistics=st, logit=logit, device=DEV).fit(dim=F - Rn, alpha=ALPHA)
        assert f.dim == F - Rn and f._dev[0].shape == ((Rn + 15) // 16 * 16, (F + 15) // 16 * 16)
        q = R.params(f.params)
        Rt, il, mu0 = (t.cpu().numpy() for t in f._dev)
        assert np.array_equal(Rt[:Rn, :F], q['Rt']) and np.array_equal(il[:Rn], q['inv_lambda']) and np.array_equal(mu0[:F], q['mu0'])
        assert not Rt[Rn:].any() and not Rt[:, F:].any() and not il[Rn:].any() and not mu0[F:].any()        # zero padding
        x = np.concatenate([d['x_in'], d['x_ood']])
        neg = logit == 'energy'
        ref = R.score(x, q, logit=d['logit'], alpha=ALPHA, negate=neg)
        f32 = R.score(x, q, np.float32, logit=d['logit'], alpha=ALPHA, negate=neg)
        _CASES[key] = {'f': f, 'q': q, 'x': x, 'logit': d['logit'], 'ref': ref, 'bounds': R.bounds(ref, f32)}
    return _CASES[key]


def _score(f, x, logit, B=3, seed=1, dtype=torch.float32):
    """rows x through a pyramid -> the three keys of the live rows, in the order of x; the padding is checked"""
    lv, an, cnt, live = _place(x, B, seed=seed, dtype=dtype)
    out = f.score(lv, an, cnt, logit_score=_logits(logit, live))
    torch.cuda.synchronize()
    assert set(out) == set(R.KEYS)
    got = {}
    for k in R.KEYS:
        assert out[k].dtype == torch.float32 and out[k].shape == an.shape
        v = out[k].cpu().numpy()
        assert (v[~live] == 0).all(), k
        got[k] = v[live]
    return got


def _check(got, c, name, rows=slice(None)):
    for k in R.KEYS:
        e32, bnd = c['bounds'][k]
        err = np.abs(got[k] - c['ref'][k][rows]).max()
        print('%s %s: %d rows, max |value| %.3g, device error %.2e, E32 %.2e, bound %.2e' % (name, k, len(got[k]), np.abs(c['ref'][k]).max(), err, e32, bnd))
        assert err <= bnd, (name, k, err, bnd)
    assert (got['residual'] <= 0).all() and (got['partial_mahalanobis'] <= 0).all(), name


def _eq(a, b):
    return all(torch.equal(a[k], b[k]) for k in a) and set(a) == set(b)


# ---- accuracy, every width -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F,Rn', [(F, Rn) for F in WIDTHS for Rn in (1, ODD[F], F)])
def test_accuracy_every_width(F, Rn):
    c = _case(F, Rn)
    _check(_score(c['f'], c['x'], c['logit'], B=5), c, 'F %d F - D %d' % (F, Rn))
    # the OOD rows lie further out than the in-distribution rows (the score does its job on the seeded draw)
    assert np.median(c['ref']['residual'][N_Q:]) < np.median(c['ref']['residual'][:N_Q])


def test_max_logit_keeps_the_sign():
    c = _case(88, 44, 'max_logit')
    got = _score(c['f'], c['x'][:200], c['logit'][:200])
    _check(got, c, 'F 88 max_logit', slice(0, 200))
    e = _score(_case(88, 44)['f'], c['x'][:200], c['logit'][:200])
    assert np.array_equal(got['residual'], e['residual']) and np.array_equal(got['partial_mahalanobis'], e['partial_mahalanobis'])
    r = -got['residual']
    assert np.array_equal(got['vim'], c['logit'][:200] - np.float32(ALPHA) * r)                 # the two roundings, on the device's own r
    assert np.array_equal(e['vim'], -c['logit'][:200] - np.float32(ALPHA) * r)


# ---- row counts around the tiling --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F,Rn', [(88, 44), (288, 288)])
def test_row_counts_around_the_tiling(F, Rn):
    c = _case(F, Rn)
    for n in ROW_COUNTS:
        for B in (1, 2):
            got = _score(c['f'], c['x'][N_Q - 3:N_Q - 3 + n], c['logit'][N_Q - 3:N_Q - 3 + n], B=B, seed=n)
            _check(got, c, 'F %d rows %d B %d' % (F, n, B), slice(N_Q - 3, N_Q - 3 + n))


def test_without_alpha_or_logit_there_is_no_vim():
    from ood_object_detection_amd.ood_features import SubspaceFeatureOOD
    c = _case(64, 44)
    lv, an, cnt, live = _place(c['x'][:50], 2)
    ls = _logits(c['logit'][:50], live)
    full = c['f'].score(lv, an, cnt, logit_score=ls)
    assert set(c['f'].score(lv, an, cnt)) == {'residual', 'partial_mahalanobis'}
    g = SubspaceFeatureOOD(64, C, A, statistics=_statistics(64)[1], device=DEV).fit(dim=20)
    assert g.alpha is None
    out = g.score(lv, an, cnt, logit_score=ls)
    assert set(out) == {'residual', 'partial_mahalanobis'} and all(torch.equal(out[k], full[k]) for k in out)
    assert set(g.fit(dim=20, alpha=ALPHA).score(lv, an, cnt, logit_score=ls)) == set(R.KEYS)
    with pytest.raises(RuntimeError, match='fit'):
        SubspaceFeatureOOD(64, C, A, device=DEV).score(lv, an, cnt)
    with pytest.raises(ValueError):
        c['f'].score(lv, None)
    with pytest.raises(ValueError, match='logit_score'):
        c['f'].score(lv, an, cnt, logit_score=ls[:, :-1])


# ---- bitwise equalities ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F,Rn', [(64, 44), (288, 100)])
def test_bfloat16_against_its_widening(F, Rn):
    c = _case(F, Rn)
    lv, an, cnt, live = _place(c['x'][:130], 3, dtype=torch.bfloat16)
    ls = _logits(c['logit'][:130], live)
    a = c['f'].score(lv, an, cnt, logit_score=ls)
    b = c['f'].score(lv.float(), an, cnt, logit_score=ls)
    torch.cuda.synchronize()
    assert _eq(a, b)
    assert float(a['residual'].abs().max()) > 0


@pytest.mark.parametrize('F,Rn', [(88, 44), (224, 224)])
def test_strided_levels_against_a_packed_tensor(F, Rn):
    c = _case(F, Rn)
    rs = np.random.RandomState(F)
    B, hw = 3, ((6, 5), (3, 3), (2, 1))
    P = sum(h * w for h, w in hw)
    packed = torch.from_numpy(rs.normal(size=(B, P, F)).astype(np.float32)).to(DEV)
    levels, at = [], 0
    for h, w in hw:                                                       # every level in a buffer with padded cells and images
        buf = torch.full((B + 1, h, w, F + 8), 55.0, device=DEV)
        buf[:B, :, :, :F] = packed[:, at:at + h * w].reshape(B, h, w, F)
        levels.append(buf[:B, :, :, :F].permute(0, 3, 1, 2))
        at += h * w
    assert not levels[0].is_contiguous(memory_format=torch.channels_last)
    an = torch.from_numpy(np.stack([rs.permutation(A * P)[:40] for _ in range(B)]).astype(np.int64)).to(DEV)
    cnt = torch.tensor([40, 17, 0], dtype=torch.int64, device=DEV)
    wide = torch.from_numpy(rs.normal(size=(B, 81)).astype(np.float32)).to(DEV)
    ls = wide[:, 1::2]                                                    # a strided logit score
    a = c['f'].score(levels, an, cnt, logit_score=ls)
    b = c['f'].score(packed, an, cnt.int(), logit_score=ls.contiguous())
    torch.cuda.synchronize()
    assert _eq(a, b)
    assert bool((a['vim'][2] == 0).all()) and bool((a['vim'][1, 17:] == 0).all()) and bool((a['vim'][0] != 0).all())
    # every cell: score_cells against score with the dense anchor index and A = 1
    from ood_object_detection_amd.ood_features import SubspaceFeatureOOD
    one = SubspaceFeatureOOD(F, C, 1, device=DEV)
    one.load_state_dict(dict(c['f'].state_dict(), num_anchors=1))
    cells = one.score_cells(levels)
    dense = one.score(packed, torch.arange(P, device=DEV).repeat(B, 1))
    assert set(cells) == {'residual', 'partial_mahalanobis'} and cells['residual'].shape == (B, P) and _eq(cells, dense)
    assert _eq(c['f'].score_cells(levels), cells)                         # score_cells does not look at num_anchors
    picked = {k: torch.gather(cells[k], 1, an // A) for k in cells}
    live = torch.arange(40, device=DEV)[None, :] < cnt[:, None]
    assert all(torch.equal(picked[k][live], a[k][live]) for k in picked)


@pytest.mark.parametrize('F,Rn', [(64, 1), (160, 100), (288, 288)])
def test_one_call_against_one_call_per_image_and_repeats(F, Rn):
    c = _case(F, Rn)
    lv, an, cnt, live = _place(c['x'][:4 * 37 - 9], 4)
    ls = _logits(c['logit'][:live.sum()], live)
    whole = c['f'].score(lv, an, cnt, logit_score=ls)
    again = c['f'].score(lv, an, cnt, logit_score=ls)
    parts = [c['f'].score(lv[b:b + 1], an[b:b + 1], cnt[b:b + 1], logit_score=ls[b:b + 1]) for b in range(4)]
    torch.cuda.synchronize()
    assert _eq(whole, again)
    assert _eq(whole, {k: torch.cat([p[k] for p in parts], 0) for k in whole})


def test_graph_replay_of_calibrate_and_score():
    from ood_object_detection_amd.ood_features import SubspaceFeatureOOD
    d, st = _statistics(112)
    f = SubspaceFeatureOOD(112, C, A, statistics=st, device=DEV).fit(dim=112 - 44, alpha=ALPHA)
    c = _case(112, 44)
    lv, an, cnt, live = _place(c['x'][:300], 4)
    ls = _logits(c['logit'][:300], live)
    f.calibrate(lv, an, cnt, ls)
    eager = f.score(lv, an, cnt, logit_score=ls)
    torch.cuda.synchronize()
    first = f.calibration()
    assert first[0] == 300
    f.reset_calibration()
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            f.calibrate(lv, an, cnt, ls)
            out = f.score(lv, an, cnt, logit_score=ls)
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    assert f.calibration() == (0, 0.0, 0.0)                               # a capture runs nothing
    g.replay()
    torch.cuda.synchronize()
    assert f.calibration() == first and _eq(out, eager)
    for k in out:
        out[k].fill_(-1.0)
    g.replay()
    torch.cuda.synchronize()
    n, s_t, s_r = f.calibration()
    assert n == 600 and _eq(out, eager)
    f.reset_calibration()
    f.calibrate(lv, an, cnt, ls)
    f.calibrate(lv, an, cnt, ls)
    assert f.calibration() == (n, s_t, s_r)                               # two eager calls: the same bits as two replays


# ---- calibration -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F,Rn,logit', [(64, 44, 'energy'), (288, 100, 'max_logit')])
def test_calibration(F, Rn, logit):
    from ood_object_detection_amd.ood_features import SubspaceFeatureOOD
    c = _case(F, Rn, logit)
    f = SubspaceFeatureOOD(F, C, A, statistics=_statistics(F)[1], logit=logit, device=DEV).fit(dim=F - Rn)
    assert f.alpha is None
    sign = -1.0 if logit == 'energy' else 1.0
    t_all = sign * c['logit'].astype(np.float64)
    total_n, total_t, total_r, total_abs = 0, 0.0, 0.0, 0.0
    for lo, n, B in ((0, 1, 1), (1, 129, 2), (130, 870, 7)):               # 1, then 3 and 19 workgroups' worth of rows
        lv, an, cnt, live = _place(c['x'][lo:lo + n], B, seed=lo)
        K = an.shape[1]
        wide = torch.full((B, 2 * K + 1), 555.0, device=DEV)
        ls = wide[:, 1::2]                                                # a strided view
        ls.copy_(_logits(c['logit'][lo:lo + n], live))
        f.calibrate(lv, an, cnt, ls)
        r = -f.score(lv, an, cnt)['residual'].cpu().numpy()[live].astype(np.float64)            # the device's own r: bit-equal in both
        total_n += n
        total_t += t_all[lo:lo + n].sum()
        total_r += r.sum()
        total_abs += np.abs(t_all[lo:lo + n]).sum()
    n, s_t, s_r = f.calibration()
    print('F %d %s: n %d, sum t %.17g (numpy %.17g), sum r %.17g (numpy of the device r %.17g)' % (F, logit, n, s_t, total_t, s_r, total_r))
    assert n == total_n == 1000
    assert abs(s_t - total_t) <= n * 2.0 ** -50 * total_abs
    assert abs(s_r - total_r) <= n * 2.0 ** -50 * total_r                   # r agrees bitwise between calibrate and score
    ref_r = c['ref']['r'].sum()
    assert abs(s_r - ref_r) <= n * 2.0 ** -50 * ref_r + n * c['bounds']['residual'][1]
    if s_t > 0:
        assert f.finish_calibration().alpha == s_t / s_r
        lv, an, cnt, live = _place(c['x'][:20], 1)
        assert 'vim' in f.score(lv, an, cnt, logit_score=_logits(c['logit'][:20], live))
    else:
        with pytest.raises(ValueError, match='threshold'):
            f.finish_calibration()
        assert f.alpha is None
    assert (s_t > 0) == (logit == 'max_logit')                              # the seeded logit scores have mean 2: t = -2 for 'energy'


def test_finish_calibration_refusals():
    from ood_object_detection_amd.ood_features import SubspaceFeatureOOD
    c = _case(64, 44)
    f = SubspaceFeatureOOD(64, C, A, statistics=_statistics(64)[1], device=DEV)
    lv, an, cnt, live = _place(c['x'][:30], 2)
    with pytest.raises(RuntimeError, match='fit'):
        f.calibrate(lv, an, cnt, _logits(c['logit'][:30], live))
    f.fit(dim=20)
    with pytest.raises(ValueError, match='no rows'):
        f.finish_calibration()
    f.calibrate(lv, an, torch.zeros_like(cnt), _logits(c['logit'][:30], live))
    assert f.calibration() == (0, 0.0, 0.0)
    with pytest.raises(ValueError, match='no rows'):
        f.finish_calibration()
    f.calibrate(lv, an, cnt, _logits(np.abs(c['logit'][:30]), live))        # energies > 0: t = -energy < 0
    n, s_t, s_r = f.calibration()
    assert n == 30 and s_t < 0 < s_r
    with pytest.raises(ValueError, match='alpha'):
        f.finish_calibration()
    f.reset_calibration()
    f.calibrate(lv, an, cnt, _logits(-np.abs(c['logit'][:30]), live))
    assert f.finish_calibration().alpha == f.calibration()[1] / f.calibration()[2] > 0
    with pytest.raises(ValueError, match='logit_score'):
        f.calibrate(lv, an, cnt, _logits(c['logit'][:30], live).double())


# ---- statistics and state ----------------------------------------------------------------------------------------------------------
def test_shared_statistics_against_separately_filled_objects():
    from ood_object_detection_amd.ood_features import FeatureOOD, SubspaceFeatureOOD
    F = 88
    d, _ = _statistics(F)
    rs = np.random.RandomState(9)
    lv, an, cnt, live = _place(d['x_fit'][:600], 3)
    det = torch.zeros(3, an.shape[1], 6, device=DEV)
    det[..., 5] = torch.from_numpy(rs.randint(1, C + 1, live.shape).astype(np.float32)).to(DEV)
    levels = [lv.unsqueeze(2).permute(0, 3, 1, 2)]                        # [B, F, P, 1]
    maha = FeatureOOD(F, C, A, DEV)
    sub = SubspaceFeatureOOD(F, C, A, statistics=maha, device=DEV)
    sub.add_detections(levels, det, an, cnt)                              # one pass fills both
    maha2 = FeatureOOD(F, C, A, DEV)
    maha2.add_detections(levels, det, an, cnt)
    sub2 = SubspaceFeatureOOD(F, C, A, device=DEV)
    sub2.add_detections(levels, det, an, cnt)
    torch.cuda.synchronize()
    assert int(maha.n_c.sum()) == 600
    for a, b, c_ in zip(maha._stats, maha2._stats, sub2.statistics._stats):
        assert torch.equal(a, b) and torch.equal(a, c_)
    maha.fit(), maha2.fit(), sub.fit(explained=0.9, alpha=ALPHA), sub2.fit(explained=0.9, alpha=ALPHA)
    assert sub.dim == sub2.dim and 0 < sub.dim < F - 1
    q, an_q, cnt_q, live_q = _place(d['x_ood'][:100], 2)
    ls = _logits(d['logit'][:100], live_q)
    assert _eq(sub.score(q, an_q, cnt_q, logit_score=ls), sub2.score(q, an_q, cnt_q, logit_score=ls))
    assert _eq(maha.score(q, an_q, cnt_q), maha2.score(q, an_q, cnt_q))
    sub.clear()
    assert int(maha.n_c.sum()) == 0 and sub._dev is None


def test_state_dict_round_trip_and_merge():
    from ood_object_detection_amd.ood_features import SubspaceFeatureOOD
    c = _case(160, 100, 'max_logit')
    f = SubspaceFeatureOOD(160, C, A, statistics=_statistics(160)[1], logit='max_logit', device=DEV).fit(dim=60)
    lv, an, cnt, live = _place(c['x'][:90], 2)
    ls = _logits(c['logit'][:90], live)
    f.calibrate(lv, an, cnt, ls)
    f.finish_calibration()
    sd = f.state_dict()
    assert sd['dim'] == 60 and sd['logit'] == 'max_logit' and sd['alpha'] == f.alpha and sd['calibration'] == f.calibration() and sd['floor'] == 1e-6
    g = SubspaceFeatureOOD(160, C, A, device=DEV).load_state_dict(sd)     # (logit comes from the state)
    assert (g.dim, g.alpha, g.logit, g.calibration()) == (60, f.alpha, 'max_logit', f.calibration())
    assert _eq(f.score(lv, an, cnt, logit_score=ls), g.score(lv, an, cnt, logit_score=ls))
    with pytest.raises(ValueError):
        SubspaceFeatureOOD(64, C, A, device=DEV).load_state_dict(sd)
    # merge_: statistics and calibration counters add up; the fit is dropped
    h = SubspaceFeatureOOD(160, C, A, device=DEV).load_state_dict(sd)
    h.merge_(g)
    assert h._dev is None and h.alpha is None and int(h.statistics.n_c.sum()) == 2 * N_FIT
    assert h.calibration() == (2 * sd['calibration'][0], 2 * sd['calibration'][1], 2 * sd['calibration'][2])
    assert torch.equal(h.statistics.S, 2 * g.statistics.S)


def test_outputs_leave_their_guard_regions_untouched():
    from ood_object_detection_amd import _lib
    F, Rn = 288, 100
    c = _case(F, Rn)
    f = c['f']
    lib = _lib.load()
    Rt, il, mu0 = f._dev
    for n, B in ((1, 1), (47, 1), (49, 1), (130, 2)):
        lv, an, cnt, live = _place(c['x'][:n], B)
        K = an.shape[1]
        ls = _logits(c['logit'][:n], live)
        G = 256
        outs = [torch.full((B * K + G,), -12345.5, device=DEV) for _ in range(3)]
        dt, B_, P, table, keep = f._table(lv)
        st = torch.cuda.current_stream(DEV).cuda_stream
        rc = lib.effdet_feature_subspace_score(st, dt, *table, F, A, B, K, an.data_ptr(), cnt.data_ptr(), 0, Rt.data_ptr(), il.data_ptr(),
                                               mu0.data_ptr(), Rt.shape[0], ls.data_ptr(), K, 1, 1, ALPHA, *[o.data_ptr() for o in outs])
        assert rc == 0
        torch.cuda.synchronize()
        ref = f.score(lv, an, cnt, logit_score=ls)
        for o, k in zip(outs, R.KEYS):
            assert torch.equal(o[:B * K].reshape(B, K), ref[k]) and bool((o[B * K:] == -12345.5).all()), k
        need = lib.effdet_feature_subspace_workspace_bytes(B * K)
        ws = torch.full((need + G,), 0xA5, dtype=torch.uint8, device=DEV)
        cn = torch.zeros(1 + 4, dtype=torch.int64, device=DEV)
        sm = torch.zeros(2 + 4, dtype=torch.float64, device=DEV)
        rc = lib.effdet_feature_subspace_calibrate(st, dt, *table, F, A, B, K, an.data_ptr(), cnt.data_ptr(), 0, Rt.data_ptr(), mu0.data_ptr(),
                                                   Rt.shape[0], ls.data_ptr(), K, 1, 1, cn.data_ptr(), sm.data_ptr(), ws.data_ptr(), need)
        assert rc == 0
        torch.cuda.synchronize()
        assert int(cn[0]) == n and not bool(cn[1:].any()) and not bool(sm[2:].any()) and bool((ws[need:] == 0xA5).all())


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def _packed(levels):
    B, F = levels[0].shape[:2]
    return torch.cat([t.permute(0, 2, 3, 1).reshape(B, -1, F) for t in levels], 1)


def test_end_to_end_d0():
    from _models import seeded_model
    from _seeded import seeded_array
    from ood_object_detection_amd import ood
    from ood_object_detection_amd.effdet.bench import DetBenchPredict
    from ood_object_detection_amd.ood_features import FeatureOOD, KNNFeatureOOD, SubspaceFeatureOOD
    from ood_object_detection_amd.serving import PipelinedPredict
    model, cfg, _, _ = seeded_model('tf_efficientdet_d0', 128, 3, seed=21, cls_bias=-2.0)
    model = model.to(DEV).float()
    x = torch.from_numpy(seeded_array(22, 'input', (4, 3, 128, 128))).to(DEV)
    plain = DetBenchPredict(model, streams=1).to(DEV)
    det0 = plain(x).clone()
    cnt0 = plain.last_count.clone()
    ai0 = plain.last_ood['anchor_index'].clone()
    energy0 = plain.last_ood['energy'].clone()
    n_det = int(cnt0.sum())
    assert n_det > 0
    na = plain.anchors.get_anchors_per_location()
    levels = model(x, mode='fpn')[1]
    maha = FeatureOOD(cfg.fpn_channels, 3, na, DEV)
    sub = SubspaceFeatureOOD(cfg.fpn_channels, 3, na, statistics=maha, device=DEV)
    sub.add_detections(levels, det0, ai0, cnt0)                           # one pass: both scorers
    maha.fit(shrinkage=0.05)
    knn = KNNFeatureOOD(cfg.fpn_channels, na, 4096, k=3, num_classes=3, device=DEV)
    knn.add_detections(levels, det0, ai0, cnt0)
    knn.fit()
    sub.fit()
    assert sub.dim == cfg.fpn_channels // 2
    # alpha by ViM's rule where the detections allow it: the mean log-sum-exp of these weak detections decides
    sub.calibrate(levels, ai0, cnt0, energy0)
    n, s_t, s_r = sub.calibration()
    live = (np.arange(det0.shape[1])[None, :] < cnt0.cpu().numpy()[:, None])
    assert n == n_det and abs(s_t + energy0.cpu().numpy()[live].astype(np.float64).sum()) <= n * 2.0 ** -50 * np.abs(energy0.cpu().numpy()[live]).sum()
    if s_t > 0:
        assert sub.finish_calibration().alpha == s_t / s_r
    else:
        with pytest.raises(ValueError, match='threshold'):
            sub.finish_calibration()
    before = DetBenchPredict(model, streams=1, feature_ood=[maha, knn]).to(DEV)
    det1 = before(x).clone()
    ood1 = {k: v.clone() for k, v in before.last_ood.items()}
    # without alpha: two new keys
    sub.fit()
    three = DetBenchPredict(model, streams=1, feature_ood=[maha, knn, sub]).to(DEV)
    three(x)
    assert set(three.last_ood) == set(ood1) | {'residual', 'partial_mahalanobis'}
    sub.fit(alpha=0.5)
    det2 = three(x)
    torch.cuda.synchronize()
    assert torch.equal(det2, det1) and torch.equal(det1, det0) and torch.equal(three.last_count, cnt0)
    assert set(three.last_ood) == set(ood1) | set(sub.KEYS)
    for k in ('energy', 'max_logit', 'anchor_index') + maha.KEYS + knn.KEYS:
        assert torch.equal(three.last_ood[k], ood1[k]), k
    got = {k: three.last_ood[k].clone() for k in sub.KEYS}
    assert got['vim'].shape == (4, three.max_det_per_image) and got['vim'].dtype == torch.float32
    with pytest.raises(ValueError, match='residual'):
        DetBenchPredict(model, feature_ood=(sub, SubspaceFeatureOOD(cfg.fpn_channels, 3, na, device=DEV)))
    # the restatement on the rows the index names, read from the engine's own pyramid
    pyr = _packed(three.model._engine.pyramid_views()).float().cpu().numpy()
    cell = ai0.cpu().numpy() // na
    rows = pyr[np.arange(4)[:, None].repeat(det0.shape[1], 1)[live], cell[live]]
    q = R.params(sub.params)
    e = energy0.cpu().numpy()[live]
    ref, f32 = R.score(rows, q, logit=e, alpha=0.5), R.score(rows, q, np.float32, logit=e, alpha=0.5)
    for k, (e32, bnd) in R.bounds(ref, f32).items():
        err = np.abs(got[k].cpu().numpy()[live] - ref[k]).max()
        print('end to end %s: %d detections, device error %.2e, E32 %.2e, bound %.2e' % (k, n_det, err, e32, bnd))
        assert err <= bnd, (k, err, bnd)
        assert bool((got[k].cpu()[torch.from_numpy(~live)] == 0).all()), k
    # logit='max_logit' reads the other gathered key
    sub_m = SubspaceFeatureOOD(cfg.fpn_channels, 3, na, statistics=maha, logit='max_logit', device=DEV).fit(alpha=0.5)
    bench_m = DetBenchPredict(model, streams=1, feature_ood=sub_m).to(DEV)
    bench_m(x)
    r = -got['residual']
    assert torch.equal(bench_m.last_ood['residual'], got['residual'])
    assert torch.equal(bench_m.last_ood['vim'][torch.from_numpy(live)], (bench_m.last_ood['max_logit'] - 0.5 * r)[torch.from_numpy(live)])
    # two sub-batch streams, and the serving pipeline with and without graphs
    two = DetBenchPredict(model, streams=2, feature_ood=[maha, knn, sub]).to(DEV)
    det3 = two(x)
    torch.cuda.synchronize()
    assert torch.equal(det3, det0) and all(torch.equal(two.last_ood[k], three.last_ood[k]) for k in three.last_ood if not k.startswith('anchor_'))
    for graphs in (False, True):
        pipe = PipelinedPredict(model, in_flight=2, graphs=graphs, feature_ood=[maha, knn, sub])
        det4, cnt4, ood4 = pipe.result(pipe.submit(x))
        assert torch.equal(det4, det0) and torch.equal(cnt4, cnt0)
        for k in sub.KEYS + knn.KEYS + maha.KEYS:
            assert torch.equal(ood4[k], three.last_ood[k]), (graphs, k)
    # the score feeds the evaluator without a conversion
    ev = ood.OODEvaluator(4 * three.max_det_per_image, 4 * three.max_det_per_image, DEV)
    ev.add_detections(got['vim'], cnt0, False)
    ev.add_detections(got['vim'] - 1.0, cnt0, True)
    res = ev.evaluate()
    assert res['n_in'] == res['n_ood'] == n_det
