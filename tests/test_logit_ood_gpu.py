"""ood_logits.LogitOOD (csrc/logit_ood.hip) against the numpy restatement of tests/_logit_ood_ref.py.

Inputs (`_logit_ood_ref.inputs`): logits 2 N(0, 1) - 3 with +5 on one random class of every in-distribution row and +1 on one of
every "OOD" row, rounded to float32; 2048 fit rows (added on the device), 500 + 500 rows to score.

Bounds.  Every float key: within 4 E32 + 1e-7 max |value| of the float64 restatement, per key and case; E32 is the float32
restatement's own error on the same inputs, and both sides start from the SAME float32 log D / kl_inf / mu / inv_sigma (the
device's `params` rounded as `fit` uploads them).  Both terms come from the restatement over the whole case of 1000 rows, never from
the device; a test that scores a subset of those rows keeps the case's bound.  predicted_class has no exclusions; kl_class must
equal the float64 restatement's choice except on rows whose best and second-best kl differ by less than twice the case's
kl_matching bound (at most 1 % of a case; the share is printed and asserted).  Every case prints E32 and the device error before it
asserts.  Measured on an MI355X: see the accuracy table of DESIGN.md §8."""
import numpy as np
import pytest
import torch

import _logit_ood_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CLASSES = (1, 2, 7, 15, 16, 17, 90, 150, 300, 520, 1024)               # the issue's list, and one size in each of the kernel's other forms
ROW_COUNTS = (1, 15, 16, 17, 63, 64, 65)                               # around the 16-row workgroup (17: one more than the tile)
N_FIT, N_Q = 2048, 500
_CASES = {}


def _place(z, B, seed=0, dtype=torch.float32):
    """n rows -> logits [B, N, C] (a strided view: padded images, anchors and classes) that hold them at shuffled anchors among other
    values, anchors [B, K] and count [B] (the last images hold the remainder, so count < K on some): row (b, j) is z[b * K + j]"""
    n, C = z.shape
    K = -(-n // B)
    N = K + 5
    rs = np.random.RandomState(n + 7 * B + seed)
    wide = rs.normal(size=(B + 1, N + 2, C + 3)).astype(np.float32)
    anchor = np.stack([rs.permutation(N)[:K] for _ in range(B)])
    count = np.clip(n - K * np.arange(B), 0, K).astype(np.int32)
    zs = np.zeros((B * K, C), np.float32)
    zs[:n] = z
    live = np.arange(K)[None, :] < count[:, None]
    wide[:B, :N, :C][np.arange(B)[:, None].repeat(K, 1)[live], anchor[live]] = zs.reshape(B, K, C)[live]
    lg = torch.from_numpy(wide).to(DEV).to(dtype)[:B, :N, :C]
    return lg, torch.from_numpy(anchor.astype(np.int64)).to(DEV), torch.from_numpy(count).to(DEV), live


def _new(C, T=1.0, top_m=10):
    from ood_object_detection_amd.ood_logits import LogitOOD
    return LogitOOD(C, temperature=T, top_m=top_m, device=DEV)


def _fill(f, z_fit):
    """the fit rows in two calls: indexed (3 images), then dense (one image)"""
    lg, an, cnt, live = _place(z_fit[:800], 3)
    f.add(lg, an, cnt)
    f.add(torch.from_numpy(z_fit[800:]).to(DEV)[None])
    return f


def _case(C, T=1.0):
    """the fitted scorer of (C, T), its float32 parameters and the 1000 rows to score; left unchanged"""
    if (C, T) not in _CASES:
        d = R.inputs(C, N_FIT, N_Q)
        f = _fill(_new(C, T), d['z_fit']).fit()
        torch.cuda.synchronize()
        assert int(f.n_c.sum()) == N_FIT
        q = R.params(f.params)
        log_d, kl_inf, mu, isg = (t.cpu().numpy() for t in f._dev)
        Cp = (C + 15) // 16 * 16
        assert log_d.shape == (Cp, Cp) and np.array_equal(log_d[:C, :C], q['log_d']) and np.array_equal(kl_inf[:C], q['kl_inf'])
        assert not log_d[C:].any() and not log_d[:, C:].any() and np.isinf(kl_inf[C:]).all()            # zero padding
        assert np.array_equal(mu, q['mu']) and np.array_equal(isg, q['inv_sigma'])
        _CASES[(C, T)] = {'f': f, 'q': q, 'z': np.concatenate([d['z_in'], d['z_ood']]), 'd': d, 'refs': {}}
    return _CASES[(C, T)]


def _ref(c, top_m):
    if top_m not in c['refs']:
        f = c['f']
        kw = dict(T=f.temperature, gamma=f.gamma, top_m=top_m, q=c['q'])
        ref = R.score(c['z'], **kw)
        c['refs'][top_m] = (ref, R.bounds(ref, R.score(c['z'], np.float32, **kw)))
    return c['refs'][top_m]


def _score(f, z, B=3, seed=1, dtype=torch.float32):
    """rows z through strided logits -> the keys of the live rows, in the order of z; the padding is checked"""
    lg, an, cnt, live = _place(z, B, seed=seed, dtype=dtype)
    out = f.score(lg, an, cnt)
    torch.cuda.synchronize()
    got = {}
    for k, t in out.items():
        assert t.shape == an.shape and t.dtype == (torch.int64 if k.endswith('class') else torch.float32), k
        v = t.cpu().numpy()
        assert (v[~live] == (-1 if k.endswith('class') else 0)).all(), k
        got[k] = v[live]
    return got


def _check(got, c, top_m, name, rows=slice(None)):
    ref, bounds = _ref(c, top_m)
    assert set(got) == set(R.KEYS)
    for k in R.FLOAT_KEYS:
        e32, bnd = bounds[k]
        err = np.abs(got[k] - ref[k][rows]).max()
        print('%s %s: %d rows, max |value| %.3g, device error %.2e, E32 %.2e, bound %.2e' % (name, k, len(got[k]), np.abs(ref[k]).max(), err, e32, bnd))
        assert err <= bnd, (name, k, err, bnd)
    assert np.array_equal(got['predicted_class'], ref['predicted_class'][rows]), name
    sure = ref['kl_margin'][rows] >= 2 * bounds['kl_matching'][1]
    share = 1.0 - sure.mean()
    print('%s kl_class: %.2f %% of the rows excluded (margin below twice the bound)' % (name, 100 * share))
    assert share <= 0.01 and np.array_equal(got['kl_class'][sure], ref['kl_class'][rows][sure]), name


def _eq(a, b):
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


def _stats_eq(f, g):
    return all(torch.equal(a, b) for a, b in zip(f._setup(), g._setup()))


# ---- accuracy ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C,T', [(C, T) for C in CLASSES for T in (1.0, 2.5)])
def test_accuracy(C, T):
    c = _case(C, T)
    for top_m in (1, 10, C + 5):
        f = _new(C, T, top_m).load_state_dict(dict(c['f'].state_dict(), top_m=top_m))
        assert f.top_m == top_m and f._dev is not None
        _check(_score(f, c['z'], B=5), c, top_m, 'C %d T %.1f top_m %d' % (C, T, top_m))
    if C in (7, 90):              # the scores do their job on the seeded draw
        ref = _ref(c, 10)[0]
        for k in ('msp', 'kl_matching'):
            assert np.median(ref[k][:N_Q]) > np.median(ref[k][N_Q:]), k
        got = _score(c['f'], c['z'], B=5)
        for k in ('msp', 'kl_matching'):
            assert np.median(got[k][:N_Q]) > np.median(got[k][N_Q:]), k


@pytest.mark.parametrize('C,T', [(17, 2.5), (90, 1.0), (1024, 1.0)])
def test_row_counts_around_the_tiling(C, T):
    c = _case(C, T)
    for n in ROW_COUNTS:
        for B in (1, 2):
            got = _score(c['f'], c['z'][N_Q - 3:N_Q - 3 + n], B=B, seed=n)
            _check(got, c, 10, 'C %d rows %d B %d' % (C, n, B), slice(N_Q - 3, N_Q - 3 + n))


def test_fitted_keys_come_with_the_fit():
    d = R.inputs(7, 64, 8)
    f = _new(7)
    lg = torch.from_numpy(d['z_in']).to(DEV)[None]
    an = torch.arange(8, device=DEV)[None]
    before = f.score(lg, an)
    assert set(before) == set(R.KEYS) - set(R.FITTED_KEYS)
    with pytest.raises(ValueError, match='no rows'):
        f.fit()
    f.add(torch.from_numpy(d['z_fit']).to(DEV)[None])
    after = f.fit().score(lg, an)
    assert set(after) == set(R.KEYS) and all(torch.equal(after[k], before[k]) for k in before)
    with pytest.raises(ValueError):
        f.score(lg, None)
    with pytest.raises(ValueError):
        f.score(lg[:, :, :6], an)
    with pytest.raises(RuntimeError):
        f.score(lg.double(), an)
    f.clear()
    assert f._dev is None and int(f.n_c.sum()) == 0 and set(f.score(lg, an)) == set(before)


# ---- extreme rows, ties, NaN --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [7, 90, 1024])
def test_extreme_rows_ties_and_a_nan_row(C):
    c = _case(C)
    f = c['f']
    z = c['z'][:64].copy()
    z[3] = -100.0
    z[3, C - 1] = 88.0                                                    # +88 and -100 in one row
    z[9] = -2.0
    z[9, [1, 2, 5]] = 3.0                                                 # exact ties: the predicted class is the lowest
    z[9, 0] = 1.0
    lg = torch.from_numpy(z).to(DEV)[None]
    a = f.score_anchors(lg)
    torch.cuda.synchronize()
    for k in R.FLOAT_KEYS:
        assert bool(torch.isfinite(a[k][0, 3])), (k, a[k][0, 3])
    assert int(a['predicted_class'][0, 3]) == C - 1 and float(a['msp'][0, 3]) == 1.0
    assert int(a['predicted_class'][0, 9]) == 1
    kw = dict(gamma=f.gamma, q=c['q'])
    for top_m in (1, 2, 3, 4):                                            # the cut falls inside the tie, at its end and beyond it
        g = _new(C, 1.0, top_m).load_state_dict(dict(f.state_dict(), top_m=top_m))
        got = g.score_anchors(lg[:, 9:10])
        ref, f32 = R.score(z[9:10], top_m=top_m, **kw), R.score(z[9:10], np.float32, top_m=top_m, **kw)
        bnd = max(R.bounds(ref, f32)['gen'][1], _ref(c, 10)[1]['gen'][1])
        err = abs(float(got['gen'][0, 0]) - ref['gen'][0])
        print('C %d ties top_m %d: gen %.9g (restatement %.9g), error %.2e, bound %.2e' % (C, top_m, float(got['gen'][0, 0]), ref['gen'][0], err, bnd))
        assert err <= bnd and int(got['predicted_class'][0, 0]) == 1
    # one NaN row among 64 leaves the other 63 rows bit-equal
    z2 = z.copy()
    z2[20, C // 2] = np.nan
    b = f.score_anchors(torch.from_numpy(z2).to(DEV)[None])
    keep = torch.arange(64, device=DEV) != 20
    assert all(torch.equal(a[k][0, keep], b[k][0, keep]) for k in a)


# ---- bitwise equalities -------------------------------------------------------------------------------------------------------------
def _levels_of(packed, C, A=3, hw=((4, 3), (2, 2), (1, 1))):
    """a packed [B, N, C] tensor (N = A * cells) -> the per-level [B, A * C, H, W] list of the class head"""
    B = packed.shape[0]
    out, at = [], 0
    for h, w in hw:
        n = h * w * A
        out.append(packed[:, at:at + n].reshape(B, h, w, A * C).permute(0, 3, 1, 2))
        at += n
    assert at == packed.shape[1]
    return out


@pytest.mark.parametrize('C,T', [(7, 2.5), (90, 1.0), (1024, 1.0)])
def test_bitwise_pairs_of_score_and_add(C, T):
    c = _case(C, T)
    f = c['f']
    z = c['z'][:3 * 51].reshape(3, 51, C)                                 # N = 51 = 3 anchors * (12 + 4 + 1) cells
    packed = torch.from_numpy(np.ascontiguousarray(z)).to(DEV)
    rs = np.random.RandomState(C)
    an = torch.from_numpy(np.stack([rs.permutation(51)[:40] for _ in range(3)]).astype(np.int64)).to(DEV)
    cnt = torch.tensor([40, 17, 0], dtype=torch.int64, device=DEV)
    wide = torch.full((4, 53, C + 8), 55.0, device=DEV)
    wide[:3, :51, :C] = packed
    strided = wide[:3, :51, :C]
    assert not strided.is_contiguous()
    base = f.score(packed, an, cnt)
    pairs = {'strided': f.score(strided, an, cnt.int()), 'levels': f.score(_levels_of(packed, C), an, cnt), 'repeat': f.score(packed, an, cnt),
             'per image': {k: torch.cat([f.score(packed[b:b + 1], an[b:b + 1], cnt[b:b + 1])[k] for b in range(3)], 0) for k in base}}
    torch.cuda.synchronize()
    for name, other in pairs.items():
        assert _eq(base, other), name
    assert bool((base['msp'][2] == 0).all()) and bool((base['kl_class'][1, 17:] == -1).all()) and bool((base['msp'][0] != 0).all())
    pb = packed.to(torch.bfloat16)
    assert _eq(f.score(pb, an, cnt), f.score(pb.float(), an, cnt))        # bfloat16 against its widening
    assert _eq(f.score(wide.to(torch.bfloat16)[:3, :51, :C], an, cnt), f.score(pb, an, cnt))
    # score_anchors against score with the identity index, and against the indexed rows
    dense = f.score_anchors(strided)
    assert dense['msp'].shape == (3, 51) and _eq(dense, f.score(packed, torch.arange(51, device=DEV).repeat(3, 1)))
    live = torch.arange(40, device=DEV)[None, :] < cnt[:, None]
    assert all(torch.equal(torch.gather(dense[k], 1, an)[live], base[k][live]) for k in base)
    # the statistics after add
    def stats(lg, *args, **kw):
        g = _new(C, T)
        g.add(lg, *args, **kw)
        return g
    s0 = stats(packed, an, cnt)
    for name, g in (('strided', stats(strided, an, cnt.int())), ('levels', stats(_levels_of(packed, C), an, cnt)), ('repeat', stats(packed, an, cnt)),
                    ('bf16', None)):
        if g is not None:
            assert _stats_eq(s0, g), name
    assert _stats_eq(stats(pb, an, cnt), stats(pb.float(), an, cnt))
    assert int(s0.n_c.sum()) == 57
    # the dense and the indexed form of the same rows, with a threshold
    thr = float(np.median(z.max(2)))
    d0, d1 = stats(strided, min_max_logit=thr), stats(packed, torch.arange(51, device=DEV).repeat(3, 1), None, min_max_logit=thr)
    assert _stats_eq(d0, d1) and int(d0.n_c.sum()) == int((z.max(2) >= np.float32(thr)).sum())
    s0.add_detections(packed, an, cnt)
    assert int(s0.n_c.sum()) == 114
    with pytest.raises(ValueError):
        s0.add_detections(packed, None, cnt)


def test_graph_replay_of_add_and_score():
    C = 90
    c = _case(C)
    lg, an, cnt, live = _place(c['z'][:300], 4)
    f = _new(C).load_state_dict(c['f'].state_dict())
    f.clear()
    f.add(lg, an, cnt)
    f.add(lg, an, cnt)
    torch.cuda.synchronize()
    twice = [t.clone() for t in f._setup()]
    f.load_state_dict(c['f'].state_dict())
    eager = f.score(lg, an, cnt)
    g_f = _new(C).load_state_dict(c['f'].state_dict())
    for t in g_f._setup():
        t.zero_()                                                           # (keeps the fit: only add is replayed)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            g_f.add(lg, an, cnt)
            out = g_f.score(lg, an, cnt)
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    assert int(g_f.n_c.sum()) == 0                                          # a capture runs nothing
    g.replay()
    torch.cuda.synchronize()
    assert int(g_f.n_c.sum()) == 300 and _eq(out, eager)
    for k in out:
        out[k].fill_(-1)
    g.replay()
    torch.cuda.synchronize()
    assert _eq(out, eager)
    assert all(torch.equal(a, b) for a, b in zip(g_f._setup(), twice))       # two eager calls: the same bits as two replays


# ---- statistics and state ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C,T', [(2, 1.0), (7, 2.5), (90, 1.0), (150, 1.0), (1024, 1.0)])
def test_fit_statistics(C, T):
    c = _case(C, T)
    f, z = c['f'], c['d']['z_fit']
    n_c, P_c, a_c, b_c = R.stats(z, C, T)
    got = [t.cpu().numpy() for t in f._setup()]
    assert np.array_equal(got[0], n_c) and got[0].sum() == N_FIT
    mz = z.max(1).astype(np.float64)
    for name, dev, ref, terms in (('a_c', got[2], a_c, np.abs(mz)), ('b_c', got[3], b_c, mz * mz)):
        err, bnd = np.abs(dev - ref).max(), N_FIT * 2.0 ** -50 * terms.sum()
        print('C %d %s: error %.2e, bound %.2e' % (C, name, err, bnd))
        assert err <= bnd, name
    ref_p, f32_p = R.softmax(z, 1.0)['p'], R.softmax(z, 1.0, np.float32)['p']
    e32 = float(np.abs(f32_p.astype(np.float64) - ref_p).max())
    bnd = float(n_c.max()) * (4 * e32 + 1e-7 * float(ref_p.max()))
    err = np.abs(got[1] - P_c).max()
    print('C %d P_c: error %.2e, E32 of p %.2e, bound %.2e (largest class %d rows)' % (C, err, e32, bnd, n_c.max()))
    assert err <= bnd
    assert np.allclose(got[1].sum(1), n_c, rtol=0, atol=1e-4 * max(n_c.max(), 1))


def test_state_dict_round_trip_and_merge():
    C = 17
    c = _case(C, 2.5)
    f = c['f']
    sd = f.state_dict()
    assert sd['num_classes'] == C and sd['temperature'] == 2.5 and sd['smoothing'] == 1e-6 and sd['std_floor'] == 1e-3
    g = _new(C).load_state_dict(sd)                                         # (temperature comes from the state)
    assert g.temperature == 2.5 and g._dev is not None and _stats_eq(f, g)
    lg, an, cnt, live = _place(c['z'][:90], 2)
    assert _eq(f.score(lg, an, cnt), g.score(lg, an, cnt))
    with pytest.raises(ValueError):
        _new(7).load_state_dict(sd)
    h = _new(C, 2.5).load_state_dict(sd)
    h.merge_(g)
    assert h._dev is None and h.params is None and int(h.n_c.sum()) == 2 * N_FIT and torch.equal(h.P_c, 2 * g.P_c) and torch.equal(h.b_c, 2 * g.b_c)
    assert set(h.score(lg, an, cnt)) == set(R.KEYS) - set(R.FITTED_KEYS)
    h.merge_(sd)
    assert int(h.n_c.sum()) == 3 * N_FIT
    with pytest.raises(ValueError):
        h.merge_(_new(7))
    # another smoothing and floor change the fitted keys only
    k1, k2 = h.fit().score(lg, an, cnt), h.fit(smoothing=1e-2, std_floor=10.0).score(lg, an, cnt)
    assert not torch.equal(k1['kl_matching'], k2['kl_matching']) and torch.equal(k1['gen'], k2['gen'])
    assert float(k2['standardized_max_logit'].abs().max()) < float(k1['standardized_max_logit'].abs().max())


def test_outputs_leave_their_guard_regions_untouched():
    from ood_object_detection_amd import _lib
    lib = _lib.load()
    for C in (7, 1024):
        c = _case(C)
        f = c['f']
        for n, B in ((1, 1), (15, 1), (17, 1), (130, 2)):
            lg, an, cnt, live = _place(c['z'][:n], B)
            K = an.shape[1]
            G = 256
            fl = [torch.full((B * K + G,), -12345.5, device=DEV) for _ in range(6)]
            ig = [torch.full((B * K + G,), -77, dtype=torch.int64, device=DEV) for _ in range(2)]
            st = torch.cuda.current_stream(DEV).cuda_stream
            head = f._head(lg)
            rc = lib.effdet_logit_ood_score(st, *head, K, an.data_ptr(), cnt.data_ptr(), 0, f.temperature, f.gamma, f.top_m,
                                            *[t.data_ptr() for t in f._dev], fl[0].data_ptr(), fl[1].data_ptr(), fl[2].data_ptr(), fl[3].data_ptr(),
                                            ig[0].data_ptr(), fl[4].data_ptr(), ig[1].data_ptr(), fl[5].data_ptr())
            assert rc == 0
            torch.cuda.synchronize()
            ref = f.score(lg, an, cnt)
            for o, k in zip(fl[:4] + [ig[0], fl[4], ig[1], fl[5]], R.KEYS):
                assert torch.equal(o[:B * K].reshape(B, K), ref[k]), k
                assert bool((o[B * K:] == (-77 if k.endswith('class') else -12345.5)).all()), k
            need = lib.effdet_logit_ood_workspace_bytes(B * K, C)
            ws = torch.full((need + G,), 0xA5, dtype=torch.uint8, device=DEV)
            nc = torch.zeros(C + 4, dtype=torch.int64, device=DEV)
            Pc = torch.zeros(C * C + 4, dtype=torch.float64, device=DEV)
            ac, bc = torch.zeros(C + 4, dtype=torch.float64, device=DEV), torch.zeros(C + 4, dtype=torch.float64, device=DEV)
            rc = lib.effdet_logit_ood_fit(st, *head, K, an.data_ptr(), cnt.data_ptr(), 0, f.temperature, 0, 0.0, nc.data_ptr(), Pc.data_ptr(),
                                          ac.data_ptr(), bc.data_ptr(), ws.data_ptr(), need)
            assert rc == 0
            torch.cuda.synchronize()
            assert int(nc[:C].sum()) == n and not bool(nc[C:].any()) and not bool(Pc[C * C:].any()) and not bool(ac[C:].any()) and not bool(bc[C:].any())
            assert bool((ws[need:] == 0xA5).all())


# ---- end to end --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['float32', 'bf16'])
def test_end_to_end_d0(mode):
    import copy
    from _models import seeded_model
    from _seeded import seeded_array
    from ood_object_detection_amd import ood
    from ood_object_detection_amd.effdet.bench import DetBenchPredict, _packed
    from ood_object_detection_amd.ood_features import FeatureOOD, KNNFeatureOOD
    from ood_object_detection_amd.ood_logits import LogitOOD
    from ood_object_detection_amd.serving import PipelinedPredict
    model, cfg, _, _ = seeded_model('tf_efficientdet_d0', 128, 3, seed=21, cls_bias=-2.0)
    model = copy.deepcopy(model).to(DEV)
    x = torch.from_numpy(seeded_array(22, 'input', (4, 3, 128, 128))).to(DEV)
    if mode == 'bf16':
        model, x = model.to(torch.bfloat16), x.to(torch.bfloat16)
    else:
        model = model.float()
    plain = DetBenchPredict(model, streams=1).to(DEV)
    det0 = plain(x).clone()
    cnt0 = plain.last_count.clone()
    ai0 = plain.last_ood['anchor_index'].clone()
    n_det = int(cnt0.sum())
    assert n_det > 0
    na = plain.anchors.get_anchors_per_location()
    levels = model(x, mode='fpn')[1]
    maha = FeatureOOD(cfg.fpn_channels, 3, na, DEV)
    maha.add_detections(levels, det0, ai0, cnt0)
    maha.fit(shrinkage=0.05)
    knn = KNNFeatureOOD(cfg.fpn_channels, na, 4096, k=3, num_classes=3, device=DEV)
    knn.add_detections(levels, det0, ai0, cnt0)
    knn.fit()
    before = DetBenchPredict(model, streams=1, feature_ood=[maha, knn]).to(DEV)
    det1 = before(x).clone()
    ood1 = {k: v.clone() for k, v in before.last_ood.items()}
    lo = LogitOOD(3, device=DEV)
    three = DetBenchPredict(model, streams=1, feature_ood=[maha, knn, lo]).to(DEV)
    three(x)
    assert set(three.last_ood) == set(ood1) | (set(lo.KEYS) - set(lo.FITTED_KEYS))            # before the fit: five new keys
    class_out, _ = model(x)
    logits = _packed(class_out, cfg.num_levels, 3)
    assert logits.dtype == (torch.float32 if mode == 'float32' else torch.bfloat16)
    lo.add_detections(class_out, ai0, cnt0)                                                   # the per-level list
    lo2 = LogitOOD(3, device=DEV)
    lo2.add_detections(logits.clone(), ai0, cnt0)
    assert _stats_eq(lo, lo2) and int(lo.n_c.sum()) == n_det
    lo.fit()
    det2 = three(x)
    torch.cuda.synchronize()
    assert torch.equal(det2, det1) and torch.equal(det1, det0) and torch.equal(three.last_count, cnt0)
    assert set(three.last_ood) == set(ood1) | set(lo.KEYS)
    for k in ('energy', 'max_logit', 'anchor_index') + maha.KEYS + knn.KEYS:
        assert torch.equal(three.last_ood[k], ood1[k]), k
    got = {k: three.last_ood[k].clone() for k in lo.KEYS}
    assert got['msp'].shape == (4, three.max_det_per_image) and got['msp'].dtype == torch.float32 and got['kl_class'].dtype == torch.int64
    with pytest.raises(ValueError, match='msp'):
        DetBenchPredict(model, feature_ood=(lo, LogitOOD(3, device=DEV)))
    # the restatement on the rows the index names
    live = (np.arange(det0.shape[1])[None, :] < cnt0.cpu().numpy()[:, None])
    lg = logits.float().cpu().numpy()
    rows = lg[np.arange(4)[:, None].repeat(det0.shape[1], 1)[live], ai0.cpu().numpy()[live]]
    if mode == 'float32':
        assert np.array_equal(rows.max(1), ood1['max_logit'].cpu().numpy()[live])             # max z is the head's own max, bit for bit
    q = R.params(lo.params)
    ref, f32 = R.score(rows, q=q), R.score(rows, np.float32, q=q)
    bnds = R.bounds(ref, f32)
    for k, (e32, bnd) in bnds.items():
        err = np.abs(got[k].cpu().numpy()[live] - ref[k]).max()
        print('end to end %s %s: %d detections, device error %.2e, E32 %.2e, bound %.2e' % (mode, k, n_det, err, e32, bnd))
        assert err <= bnd, (k, err, bnd)
        assert bool((got[k].cpu()[torch.from_numpy(~live)] == 0).all()), k
    assert np.array_equal(got['predicted_class'].cpu().numpy()[live], ref['predicted_class'])
    assert bool((got['predicted_class'].cpu()[torch.from_numpy(~live)] == -1).all())
    sure = ref['kl_margin'] >= 2 * bnds['kl_matching'][1]
    print('end to end %s kl_class: %.2f %% of %d rows excluded' % (mode, 100 * (1 - sure.mean()), n_det))
    assert np.array_equal(got['kl_class'].cpu().numpy()[live][sure], ref['kl_class'][sure])
    # two sub-batch streams, and the serving pipeline with and without graphs
    two = DetBenchPredict(model, streams=2, feature_ood=[maha, knn, lo]).to(DEV)
    det3 = two(x)
    torch.cuda.synchronize()
    assert torch.equal(det3, det0) and all(torch.equal(two.last_ood[k], three.last_ood[k]) for k in three.last_ood if not k.startswith('anchor_'))
    for graphs in (False, True):
        pipe = PipelinedPredict(model, in_flight=2, graphs=graphs, feature_ood=[maha, knn, lo])
        det4, cnt4, ood4 = pipe.result(pipe.submit(x))
        assert torch.equal(det4, det0) and torch.equal(cnt4, cnt0)
        for k in lo.KEYS + knn.KEYS + maha.KEYS:
            assert torch.equal(ood4[k], three.last_ood[k]), (graphs, k)
    # a score feeds the evaluator without a conversion
    ev = ood.OODEvaluator(4 * three.max_det_per_image, 4 * three.max_det_per_image, DEV)
    ev.add_detections(got['kl_matching'], cnt0, False)
    ev.add_detections(got['kl_matching'] - 1.0, cnt0, True)
    res = ev.evaluate()
    assert res['n_in'] == res['n_ood'] == n_det
