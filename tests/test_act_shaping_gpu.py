"""ood_shaping.ActivationShapingOOD (csrc/act_shaping.hip) against the numpy restatement of tests/_act_shaping_ref.py.

Inputs (`_act_shaping_ref.inputs`): tower values silu(N(0, 1)) on the levels 4 x 3, 2 x 2 and 1 x 1 of 3 images, taps N(0, 0.3),
weights N(0, 1 / sqrt(F)) with a bump on one class per anchor slot, bias N(0, 0.1); the towers reach the device as strided views
(padded images and channels).  A case is (F, C, A, dtype) and its rows are ALL A * 17 anchors of the 3 images.

Exact: the shaped rows of none / react / ash_p and the zero pattern of ash_b / ash_s (the device's d is bit-equal to the float32
restatement's, so the kept sets are the same), n and the histogram of a fit, the fitted c.  Bounds: every float key within
4 E32 + 1e-7 max |value| of the float64 restatement, per key and case; E32 is the float32 restatement's own error over the whole
case, never taken from the device; a test that scores a subset of the rows keeps the case's bound.  `<name>_class` equals the
float64 choice except on rows whose top-two margin is below twice the case's logit bound (at most 1 % of a case; the share is
printed and asserted).  Every case prints E32 and the device error before it asserts.  Measured on an MI355X: see DESIGN.md §8."""
import numpy as np
import pytest
import torch

import _act_shaping_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
B = 3
P = sum(h * w for h, w in R.LEVELS)
WIDTHS = (64, 88, 112, 160, 224, 288)
ROW_COUNTS = (1, 15, 16, 17, 63, 64, 65)
_CASES = {}
_REFS = {}


def _S():
    from ood_object_detection_amd.ood_shaping import ActivationShapingOOD
    return ActivationShapingOOD


def _place(tower, dtype=torch.float32, seed=0):
    """per-level NHWC arrays -> per-level [B, F, h, w] device views with channel stride 1 inside padded buffers (one more image, three
    more channels a cell), as test_logit_ood_gpu._place pads its logits"""
    out = []
    for l, x in enumerate(tower):
        b, h, w, F = x.shape
        wide = np.random.RandomState(seed + l).normal(size=(b + 1, h, w, F + 3)).astype(np.float32)
        wide[:b, :, :, :F] = x
        t = torch.from_numpy(wide).to(DEV).to(dtype)[:b, :, :, :F].permute(0, 3, 1, 2)
        assert t.stride(1) == 1 and not t.is_contiguous(memory_format=torch.channels_last)
        out.append(t)
    return out


def _case(F, C, A, bf16=False):
    """the inputs of a case, its device tower, d and the all-anchor rows; left unchanged"""
    key = (F, C, A, bf16)
    if key not in _CASES:
        d_in = R.inputs(F, C, A, B)
        tower = d_in['tower']
        if bf16:
            tower = [R.widen_bf16(R.to_bf16_bits(x)) for x in tower]
        d = R.penultimate(tower, d_in['taps'])                             # [B, P, F]
        dev = _place(tower, torch.bfloat16 if bf16 else torch.float32)
        if bf16:
            assert all(np.array_equal(t.float().permute(0, 2, 3, 1).cpu().numpy(), x) for t, x in zip(dev, tower))
        all_d = np.repeat(d.reshape(B * P, F), A, 0)
        n, sum_d, hist = R.fit_stats(all_d)                                # what a dense add sees: every cell A times
        _CASES[key] = dict(d_in, F=F, C=C, A=A, N=A * P, tower_np=tower, tower=dev, d=d, all_d=all_d,
                           all_slot=np.tile(np.arange(A), B * P), n=n, sum_d=sum_d, hist=hist,
                           c=R.react_threshold(hist, n, F, 90.0)[0])
    return _CASES[key]


def _scorer(c, method, **kw):
    s = _S()(c['F'], c['C'], c['A'], method=method, device=DEV, **kw)
    s.set_weights(c['taps'], c['W'], c['bias'])
    if s.needs_fit:
        s.add(c['tower'])
        s.fit()
    return s


def _ref(c, method, T=1.0, W=None):
    key = (c['F'], c['C'], c['A'], id(c), method, T, W is not None)
    if key not in _REFS:
        kw = dict(method=method, k=R.k_of(c['F'], 90.0), c=c['c'], T=T, gradnorm=True)
        Wm = c['W'] if W is None else W
        ref = R.score(c['all_d'], c['all_slot'], Wm, c['bias'], c['A'], **kw)
        f32 = R.score(c['all_d'], c['all_slot'], Wm, c['bias'], c['A'], dtype=np.float32, **kw)
        _REFS[key] = (ref, f32, R.bounds(ref, f32))
    return _REFS[key]


def _check(got, idx, c, method, name, T=1.0, W=None):
    """got: key (without the name prefix) -> flat array over the rows idx of the case's all-anchor list"""
    ref, f32, bnd = _ref(c, method, T, W)
    for k in R.FLOAT_KEYS:
        if k not in got:
            continue
        e32, b = bnd[k]
        err = float(np.abs(got[k] - ref[k][idx]).max())
        print('%s %s: %d rows, max |value| %.3g, device error %.2e, E32 %.2e, bound %.2e' % (name, k, len(got[k]), np.abs(ref[k]).max(), err, e32, b))
        assert err <= b, (name, k, err, b)
    sure = ref['margin'][idx] >= 2 * bnd['logits'][1]
    share = 1.0 - sure.mean()
    print('%s class: %.2f %% of the rows excluded (margin below twice the logit bound %.2e)' % (name, 100 * share, bnd['logits'][1]))
    assert share <= 0.01 and np.array_equal(got['class'][sure], ref['class'][idx][sure]), name


def _strip(s, out):
    return {k[len(s.name) + 1:] if k.startswith(s.name + '_') else k: v for k, v in out.items()}


def _all_anchors(c, seed=0):
    """every anchor of every image in a shuffled order: anchor [B, N] int64 and the rows' indices into the all-anchor list"""
    rs = np.random.RandomState(seed)
    an = np.stack([rs.permutation(c['N']) for _ in range(B)]).astype(np.int64)
    return torch.from_numpy(an).to(DEV), (np.arange(B)[:, None] * c['N'] + an).ravel()


def _score_all(s, c, method, name, T=1.0, W=None):
    """the entries form over all anchors (exact checks of the rows, bounds of the keys), then the cells form within the same bounds"""
    an, idx = _all_anchors(c)
    out = s.score(c['tower'], an, rows=True)
    dense = s.score_anchors(c['tower'])
    torch.cuda.synchronize()
    ref, f32, _ = _ref(c, method, T, W)
    x = out.pop('rows').cpu().numpy().reshape(-1, c['F'])
    x32 = f32['rows'][idx]
    if method in ('none', 'react', 'ash_p'):
        assert np.array_equal(x.view(np.uint32), x32.view(np.uint32)), (name, 'rows')
    else:
        assert np.array_equal(x == 0, x32 == 0), (name, 'zero pattern')
        if method == 'ash_b':
            assert (np.abs(x - ref['rows'][idx]) <= 1e-6 * np.abs(ref['rows'][idx])).all()
    for k, t in out.items():
        assert t.shape == an.shape and t.dtype == (torch.int64 if k.endswith('class') else torch.float32), k
    got = {k: v.cpu().numpy().ravel() for k, v in _strip(s, out).items()}
    _check(got, idx, c, method, name + ' entries', T, W)
    for k, t in dense.items():
        assert t.shape == (B, c['N']) and t.dtype == (torch.int64 if k.endswith('class') else torch.float32), k
    _check({k: v.cpu().numpy().ravel() for k, v in _strip(s, dense).items()}, np.arange(B * c['N']), c, method, name + ' cells', T, W)


# ---- accuracy ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F', [64, 288])
@pytest.mark.parametrize('method', R.METHODS)
def test_every_method(F, method):
    c = _case(F, 17, 3)
    s = _scorer(c, method, gradnorm=True)
    assert s.KEYS == ('%s_energy' % method, '%s_max_logit' % method, '%s_class' % method, 'gradnorm')
    if method == 'react':
        assert np.float32(s.c) == c['c']
    _score_all(s, c, method, 'F %d %s' % (F, method))


@pytest.mark.parametrize('bf16', [False, True])
@pytest.mark.parametrize('F', WIDTHS)
@pytest.mark.parametrize('method', ['react', 'ash_s'])
def test_every_width(F, method, bf16):
    c = _case(F, 17, 3, bf16)
    _score_all(_scorer(c, method, gradnorm=True, temperature=2.5), c, method, 'F %d %s %s' % (F, method, 'bf16' if bf16 else 'f32'), T=2.5)


@pytest.mark.parametrize('A', [3, 9])
@pytest.mark.parametrize('C', [1, 2, 16, 17, 90, 150])
def test_class_counts_and_anchor_slots(C, A):
    c = _case(64, C, A)
    for method in ('ash_s', 'react'):
        _score_all(_scorer(c, method, gradnorm=True), c, method, 'C %d A %d %s' % (C, A, method))


def test_a_thousand_classes():
    c = _case(64, 1024, 3)
    _score_all(_scorer(c, 'scale', gradnorm=True), c, 'scale', 'C 1024 scale')


@pytest.mark.parametrize('method', ['react', 'ash_b'])
def test_row_counts_around_the_tiling(method):
    c = _case(88, 17, 9)                                                   # 153 anchors an image: 65 rows fit into one
    s = _scorer(c, method, gradnorm=True)
    for n in ROW_COUNTS:
        for nb in (1, 2):
            K = -(-n // nb)
            rs = np.random.RandomState(n + nb)
            an = np.stack([rs.permutation(c['N'])[:K] for _ in range(nb)]).astype(np.int64)
            count = np.clip(n - K * np.arange(nb), 0, K).astype(np.int32)
            live = np.arange(K)[None, :] < count[:, None]
            out = s.score([t[:nb] for t in c['tower']], torch.from_numpy(an).to(DEV), torch.from_numpy(count).to(DEV), rows=True)
            torch.cuda.synchronize()
            rows = out.pop('rows').cpu().numpy()
            assert not rows[~live].any()
            got = {}
            for k, t in _strip(s, out).items():
                v = t.cpu().numpy()
                assert (v[~live] == (-1 if k == 'class' else 0)).all(), k
                got[k] = v[live]
            _check(got, (np.arange(nb)[:, None] * c['N'] + an)[live], c, method, '%s rows %d B %d' % (method, n, nb))


# ---- fit --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('F,bf16', [(64, False), (88, True), (288, False)])
def test_fit_statistics_threshold_and_dice(F, bf16):
    c = _case(F, 17, 3, bf16)
    s = _S()(F, 17, 3, method='react', dice=80.0, device=DEV)
    with pytest.raises(RuntimeError, match='set_head'):
        s.add(c['tower'])
    s.set_weights(c['taps'], c['W'], c['bias'])
    with pytest.raises(RuntimeError, match='fit'):
        s.score_anchors(c['tower'])
    with pytest.raises(ValueError, match='no rows'):
        s.fit()
    an, idx = _all_anchors(c, seed=3)
    count = torch.tensor([c['N'], 20, 0], dtype=torch.int64, device=DEV)
    s.add(c['tower'], an, count)                                           # indexed: the cells behind (N + 20) anchors
    s.add(c['tower'])                                                      # dense: every anchor
    live = (np.arange(c['N'])[None, :] < count.cpu().numpy()[:, None]).ravel()
    rows = np.concatenate([c['all_d'][idx[live]], c['all_d']])
    n, sum_d, hist = R.fit_stats(rows)
    got_n, got_sum, got_hist = int(s.n.cpu()[0]), s.sum_d.cpu().numpy(), s.hist.cpu().numpy()
    assert got_n == n == c['N'] + 20 + B * c['N'] and np.array_equal(got_hist, hist)
    scale = np.abs(rows.astype(np.float64)).sum(0)
    err = float((np.abs(got_sum - sum_d) / scale).max())
    print('F %d sum_d: %d rows, relative error %.2e (bound 1e-12)' % (F, n, err))
    assert err <= 1e-12
    s.fit()
    assert np.float32(s.c) == R.react_threshold(got_hist, got_n, F, 90.0)[0]
    masked, keep = R.dice_weight(c['W'], got_sum, got_n, 80.0)
    assert np.array_equal(s.weight, masked) and abs(keep.mean() - 0.2) < 0.01
    assert s.name == 'react_dice'
    cc = dict(c, c=np.float32(s.c))
    _score_all(s, cc, 'react', 'F %d react + dice' % F, W=masked)
    # add_targets takes the positive anchors only: the same statistics as the indexed add of those anchors
    labels = np.random.RandomState(F).randint(-2, 3, size=(B, c['N']))
    maps, at = [], 0
    for h, w in R.LEVELS:
        maps.append(torch.from_numpy(labels[:, at:at + h * w * 3].reshape(B, h, w, 3)).to(DEV))
        at += h * w * 3
    a, b = _S()(F, 17, 3, device=DEV).set_weights(c['taps'], c['W'], c['bias']), _S()(F, 17, 3, device=DEV).set_weights(c['taps'], c['W'], c['bias'])
    a.add_targets(c['tower'], maps)
    pos = labels >= 0
    K = int(pos.sum(1).max())
    an2 = np.zeros((B, K), np.int64)
    for i in range(B):
        an2[i, :pos[i].sum()] = np.nonzero(pos[i])[0]
    b.add_detections(c['tower'], torch.from_numpy(an2).to(DEV), torch.from_numpy(pos.sum(1)).to(DEV))
    assert int(a.n.cpu()[0]) == int(pos.sum()) and all(torch.equal(x, y) for x, y in zip(a._setup(), b._setup()))
    a.clear()
    assert int(a.n.cpu()[0]) == 0 and not bool(a.hist.any()) and not a.fitted


# ---- bitwise equalities -------------------------------------------------------------------------------------------------------------
def _eq(a, b):
    return set(a) == set(b) and all(torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k],
                                                b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k]) for k in a)


@pytest.mark.parametrize('F,C,A,method', [(64, 17, 3, 'ash_s'), (160, 90, 9, 'react'), (288, 2, 3, 'scale')])
def test_forms_are_bitwise_stable_across_groupings(F, C, A, method):
    c = _case(F, C, A)
    s = _scorer(c, method, gradnorm=True)
    tw = c['tower']
    dense = s.score_anchors(tw)
    for split in ((1, 2), (2, 1), (1, 1, 1)):                              # the batch in two and in three calls
        parts, at = [], 0
        for nb in split:
            parts.append(s.score_anchors([t[at:at + nb] for t in tw]))
            at += nb
        assert _eq(dense, {k: torch.cat([p[k] for p in parts], 0) for k in dense}), split
    assert _eq(dense, s.score_anchors([t.contiguous(memory_format=torch.channels_last) for t in tw]))
    an, idx = _all_anchors(c, seed=5)
    base = s.score(tw, an, rows=True)
    halves = [s.score(tw, an[:, :40], rows=True), s.score(tw, an[:, 40:], rows=True)]
    assert _eq(base, {k: torch.cat([h[k] for h in halves], 1) for k in base})
    per_image = [s.score([t[i:i + 1] for t in tw], an[i:i + 1], rows=True) for i in range(B)]
    assert _eq(base, {k: torch.cat([p[k] for p in per_image], 0) for k in base})
    assert _eq(base, s.score(tw, an, torch.full((B,), c['N'], dtype=torch.int32, device=DEV), rows=True))
    assert _eq(s.score_anchors(tw), dense)                                 # run to run


def test_bf16_tower_against_its_widening():
    c = _case(88, 17, 3, True)
    s = _scorer(c, 'ash_p', gradnorm=True)
    wide = _place(c['tower_np'], torch.float32, seed=9)
    an, _ = _all_anchors(c)
    assert _eq(s.score(c['tower'], an, rows=True), s.score(wide, an, rows=True)) and _eq(s.score_anchors(c['tower']), s.score_anchors(wide))


def test_kept_set_with_equal_values_at_the_cut():
    """The in-wave select of the k largest (wave_rows.h) where equal values meet the cut.  One 1 x 1 level, A = 1 and taps that are 1 on
    the centre and -0 elsewhere, so that d IS the tower value, its sign of zero included (-0 * 0 = -0, -0 + -0 = -0, -0 + +0 = +0), on
    the device and in the restatement alike; F = 88: two registers a lane, 24 channels live in the second.  Rows: four equal values
    at channels 3, 63, 64 and 87 below ten larger ones (positive, and once more negative), -0 at channel 40 and +0 at channel 80 below
    eleven larger ones, 88 equal values, 88 distinct ones.  k = 12, 13: inside the group (and the pair); 14: its end; 15: one past; 1 and F - 1."""
    F, C, GROUP = 88, 2, [3, 63, 64, 87]
    rs = np.random.RandomState(88)

    def row(fixed, larger, top, rest):
        """`fixed`: channel -> value; of the other channels, shuffled, `larger` get distinct values above `top`, the rest below `rest`"""
        x = np.zeros(F, np.float32)
        free = rs.permutation([j for j in range(F) if j not in fixed])
        x[free[:larger]] = top + 0.125 * (1 + np.arange(larger))
        x[free[larger:]] = rest - 0.03125 * (1 + np.arange(len(free) - larger))
        for j, v in fixed.items():
            x[j] = v
        return x

    x = np.stack([row({j: 1.0 for j in GROUP}, 10, 1.0, 1.0),           # the rest runs from 0.97 down to -1.3
                  row({j: -0.25 for j in GROUP}, 10, -0.25, -0.25),
                  row({40: -0.0, 80: 0.0}, 11, 0.0, 0.0),
                  np.full(F, 0.5, np.float32),
                  rs.normal(size=F).astype(np.float32)])
    n = len(x)
    taps = np.full((9, F), -0.0, np.float32)
    taps[4] = 1.0
    d = R.penultimate([x.reshape(n, 1, 1, F)], taps).reshape(n, F)
    assert np.array_equal(d.view(np.uint32), x.view(np.uint32)) and np.signbit(d[2, 40]) and not np.signbit(d[2, 80])
    W = rs.normal(size=(C, F)).astype(np.float32)
    tower = _place([x.reshape(n, 1, 1, F)])
    an = torch.zeros(n, 1, dtype=torch.int64, device=DEV)
    for k, group, pair in ((1, [], []), (12, [3, 63], [40]), (13, [3, 63, 64], [40, 80]), (14, GROUP, [40, 80]), (15, GROUP, [40, 80]),
                           (F - 1, GROUP, [40, 80])):
        kept = R.kept_set(d, k)                                            # the restatement keeps what this test means it to keep
        assert (kept.sum(1) == k).all() and np.array_equal(kept[3], np.arange(F) < k)
        for r in (0, 1):
            assert [j for j in GROUP if kept[r, j]] == group, (k, r)
        assert [j for j in (40, 80) if kept[2, j]] == pair, k
        p = 100.0 * (F - k) / F
        assert R.k_of(F, p) == k
        s = _S()(F, C, 1, method='ash_p', percentile=p, device=DEV).set_weights(taps, W, np.zeros(C, np.float32))
        got = s.score(tower, an, rows=True)['rows'].cpu().numpy().reshape(n, F)
        want = R.shape(d, 'ash_p', k=k, dtype=np.float32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (k, np.argwhere(got.view(np.uint32) != want.view(np.uint32)))
        assert np.array_equal(got != 0, kept & (d != 0))


def test_graph_replay_of_add_score_and_score_anchors():
    c = _case(64, 17, 3)
    s = _scorer(c, 'react', gradnorm=True)
    an, _ = _all_anchors(c, seed=2)
    count = torch.tensor([c['N'], 30, 0], dtype=torch.int32, device=DEV)
    eager, eager_dense = s.score(c['tower'], an, count), s.score_anchors(c['tower'])
    before = [t.clone() for t in s._setup()]
    s.add(c['tower'], an, count)
    s.add(c['tower'], an, count)
    torch.cuda.synchronize()
    twice = [t.clone() for t in s._setup()]
    for t, b in zip(s._setup(), before):
        t.copy_(b)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            s.add(c['tower'], an, count)
            out = s.score(c['tower'], an, count)
            dense = s.score_anchors(c['tower'])
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(s._setup(), before))       # a capture runs nothing
    for _ in range(2):
        for t in list(out.values()) + list(dense.values()):
            t.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert _eq(out, eager) and _eq(dense, eager_dense)
    assert all(torch.equal(a, b) for a, b in zip(s._setup(), twice))        # two replays: the same bits as two eager calls


def test_state_dict_round_trip_and_merge():
    c = _case(64, 17, 3)
    s = _scorer(c, 'react', dice=50.0)
    sd = s.state_dict()
    assert sd['method'] == 'react' and sd['fitted'] and sd['c'] == s.c and int(sd['n'][0]) == B * c['N']
    g = _S()(64, 17, 3, method='react', dice=50.0, device=DEV).set_weights(c['taps'], c['W'], c['bias']).load_state_dict(sd)
    assert g.fitted and g.c == s.c and np.array_equal(g.weight, s.weight) and all(torch.equal(a, b) for a, b in zip(s._setup(), g._setup()))
    an, _ = _all_anchors(c)
    assert _eq(s.score(c['tower'], an), g.score(c['tower'], an))
    with pytest.raises(ValueError):
        _S()(64, 17, 3, method='ash_p', device=DEV).load_state_dict(sd)
    g.merge_(s)
    assert not g.fitted and g.c is None and int(g.n.cpu()[0]) == 2 * B * c['N'] and torch.equal(g.hist, 2 * s.hist) and torch.equal(g.sum_d, 2 * s.sum_d)
    assert np.array_equal(g.weight, c['W'])                               # the mask goes with the fit
    with pytest.raises(RuntimeError, match='fit'):
        g.score(c['tower'], an)
    g.merge_(sd).fit()
    assert int(g.n.cpu()[0]) == 3 * B * c['N'] and g.c == s.c and np.array_equal(g.weight, s.weight)      # the same rows three times over
    with pytest.raises(ValueError):
        g.merge_(_S()(64, 17, 3, method='react', device=DEV))


def test_nan_row_and_cpu_tensors():
    c = _case(64, 17, 3)
    s = _scorer(c, 'ash_s', gradnorm=True)
    an, _ = _all_anchors(c)
    base, dense = s.score(c['tower'], an, rows=True), s.score_anchors(c['tower'])
    tower = [t.clone() for t in c['tower']]
    tower[0][1, 5, 0, 0] = float('nan')                                    # the corner (0, 0) of the 4 x 3 level of image 1
    hit = {0, 1, 3, 4}                                                     # the cells whose window holds it: (0..1, 0..1)
    out, d2 = s.score(tower, an, rows=True), s.score_anchors(tower)
    torch.cuda.synchronize()
    bad = torch.zeros(B, c['N'], dtype=torch.bool, device=DEV)
    for cell in hit:
        bad[1, cell * 3:cell * 3 + 3] = True
    bad_e = torch.gather(bad, 1, an)
    for k in out:
        if k == 'rows':
            assert bool(torch.isnan(out[k][bad_e]).all()) and torch.equal(out[k][~bad_e], base[k][~bad_e])
        elif k.endswith('class'):
            assert bool((out[k][bad_e] == -1).all()) and bool((d2[k][bad] == -1).all())
            assert torch.equal(out[k][~bad_e], base[k][~bad_e]) and torch.equal(d2[k][~bad], dense[k][~bad])
        else:
            assert bool(torch.isnan(out[k][bad_e]).all()) and bool(torch.isnan(d2[k][bad]).all()), k
            assert torch.equal(out[k][~bad_e], base[k][~bad_e]) and torch.equal(d2[k][~bad], dense[k][~bad]), k
    f = _S()(64, 17, 3, method='none', device=DEV).set_weights(c['taps'], c['W'], c['bias'])
    f.add(tower)
    assert int(f.n.cpu()[0]) == B * c['N'] - 12                            # rows with a non-finite d are skipped
    with pytest.raises(RuntimeError, match='GPU'):
        s.score([t.cpu() for t in c['tower']], an.cpu())
    with pytest.raises(ValueError):
        s.score(c['tower'], None)


def test_outputs_leave_their_guard_regions_untouched():
    from ood_object_detection_amd import _lib
    lib = _lib.load()
    c = _case(88, 17, 3)
    s = _scorer(c, 'ash_s', gradnorm=True)
    st = torch.cuda.current_stream(DEV).cuda_stream
    G = 256
    for n in (1, 5, 51):
        an, _ = _all_anchors(c, seed=n)
        an = an[:, :n].contiguous()
        dt, nb, p, table, keep = s._tower(c['tower'])
        fl = [torch.full((B * n + G,), -12345.5, device=DEV) for _ in range(3)]
        cl = torch.full((B * n + G,), -77, dtype=torch.int64, device=DEV)
        xr = torch.full((B * n * 88 + G,), -12345.5, device=DEV)
        taps, w_rows, w_tiles, bias = s._dev
        rc = lib.effdet_act_shaping_score(st, dt, *table, 88, 17, 3, B, n, an.data_ptr(), None, 0, taps.data_ptr(), w_rows.data_ptr(),
                                          bias.data_ptr(), *s._method_args(), fl[0].data_ptr(), fl[1].data_ptr(), cl.data_ptr(), fl[2].data_ptr(),
                                          xr.data_ptr())
        assert rc == 0
        torch.cuda.synchronize()
        ref = s.score(c['tower'], an, rows=True)
        for o, k in zip(fl + [cl, xr], ('ash_s_energy', 'ash_s_max_logit', 'gradnorm', 'ash_s_class', 'rows')):
            m = ref[k].numel()
            assert torch.equal(o[:m], ref[k].reshape(-1)) and bool((o[m:] == (-77 if k.endswith('class') else -12345.5)).all()), k
        need = lib.effdet_act_shaping_workspace_bytes(B * n, 88)
        ws = torch.full((need + G,), 0xA5, dtype=torch.uint8, device=DEV)
        nn_ = torch.zeros(1 + 4, dtype=torch.int64, device=DEV)
        sd = torch.zeros(88 + 4, dtype=torch.float64, device=DEV)
        hist = torch.zeros(65536 + 4, dtype=torch.int64, device=DEV)
        rc = lib.effdet_act_shaping_fit(st, dt, *table, 88, 3, B, n, an.data_ptr(), None, 0, taps.data_ptr(), nn_.data_ptr(), sd.data_ptr(),
                                        hist.data_ptr(), ws.data_ptr(), need)
        assert rc == 0
        torch.cuda.synchronize()
        assert int(nn_[0]) == B * n and not bool(nn_[1:].any()) and not bool(sd[88:].any()) and not bool(hist[65536:].any())
        assert int(hist.sum()) == B * n * 88 and bool((ws[need:] == 0xA5).all())
    N = c['N']
    fl = [torch.full((B * N + G,), -12345.5, device=DEV) for _ in range(3)]
    cl = torch.full((B * N + G,), -77, dtype=torch.int64, device=DEV)
    rc = lib.effdet_act_shaping_score_cells(st, dt, *table, 88, 17, 3, B, taps.data_ptr(), w_tiles.data_ptr(), bias.data_ptr(), *s._method_args(),
                                            fl[0].data_ptr(), fl[1].data_ptr(), cl.data_ptr(), fl[2].data_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    ref = s.score_anchors(c['tower'])
    for o, k in zip(fl + [cl], ('ash_s_energy', 'ash_s_max_logit', 'gradnorm', 'ash_s_class')):
        assert torch.equal(o[:B * N], ref[k].reshape(-1)) and bool((o[B * N:] == (-77 if k.endswith('class') else -12345.5)).all()), k


# ---- end to end --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['float32', 'bf16'])
def test_end_to_end_d0(mode):
    import copy
    from _models import seeded_model
    from _seeded import seeded_array
    from ood_object_detection_amd.effdet.bench import DetBenchPredict
    model, cfg, _, _ = seeded_model('tf_efficientdet_d0', 128, 3, seed=21, cls_bias=-2.0)
    model = copy.deepcopy(model).to(DEV)
    x = torch.from_numpy(seeded_array(22, 'input', (4, 3, 128, 128))).to(DEV)
    if mode == 'bf16':
        model, x = model.to(torch.bfloat16), x.to(torch.bfloat16)
    else:
        model = model.float()
    assert model.keep_class_tower is False
    plain = DetBenchPredict(model, streams=1).to(DEV)
    det0 = plain(x).clone()
    cnt0, ood0 = plain.last_count.clone(), {k: v.clone() for k, v in plain.last_ood.items()}
    cls0, box0 = model(x)
    cls0, box0 = [t.clone() for t in cls0], [t.clone() for t in box0]
    with pytest.raises(RuntimeError, match='keep_class_tower'):
        model._engine.class_tower_views()
    eng0 = model._engine
    n_det = int(cnt0.sum())
    assert n_det > 0
    A, F = plain.anchors.get_anchors_per_location(), cfg.fpn_channels
    S = _S()
    none = S(F, 3, A, method='none', device=DEV).set_head(model.class_net)
    react = S(F, 3, A, method='react', device=DEV).set_head(model.class_net)
    bench = DetBenchPredict(model, streams=1, feature_ood=[none, react]).to(DEV)
    assert model.keep_class_tower is True
    cls1, box1 = model(x)
    assert model._engine is not eng0 and model._engine.keep_class_tower                       # the flag rebuilt the plan
    assert all(torch.equal(a, b) for a, b in zip(cls0 + box0, list(cls1) + list(box1)))        # only a destination pointer differs
    tower = model._engine.class_tower_views()
    assert [tuple(t.shape) for t in tower] == [(4, F, s, s) for s in (16, 8, 4, 2, 1)] and tower[0].dtype == x.dtype
    react.add_detections(tower, ood0['anchor_index'], cnt0)
    assert int(react.n.cpu()[0]) == n_det
    react.fit()
    det1 = bench(x)
    torch.cuda.synchronize()
    assert torch.equal(det1, det0) and torch.equal(bench.last_count, cnt0)
    assert set(bench.last_ood) == set(ood0) | set(none.KEYS) | set(react.KEYS)
    for k in ood0:
        assert torch.equal(bench.last_ood[k], ood0[k]), k
    got = {k: bench.last_ood[k].clone() for k in none.KEYS + react.KEYS}
    with pytest.raises(ValueError, match='react_energy'):
        DetBenchPredict(model, feature_ood=[react, S(F, 3, A, method='react', device=DEV)])
    # the restatement from the downloaded tower at the counted detections
    live = np.arange(det0.shape[1])[None, :] < cnt0.cpu().numpy()[:, None]
    taps, W, bias = none._head
    d = R.penultimate([t.float().permute(0, 2, 3, 1).cpu().numpy() for t in model._engine.class_tower_views()], taps)
    an = ood0['anchor_index'].cpu().numpy()
    rows, slots = d[np.arange(4)[:, None].repeat(det0.shape[1], 1)[live], an[live] // A], an[live] % A
    ref, f32 = R.score(rows, slots, W, bias, A), R.score(rows, slots, W, bias, A, dtype=np.float32)
    bnd = R.bounds(ref, f32)
    for k in ('energy', 'max_logit'):
        mine, head = got['none_' + k].cpu().numpy()[live], ood0[k].cpu().numpy()[live]
        e_mine, e_head = np.abs(mine - ref[k]).max(), np.abs(head - ref[k]).max()
        print('end to end %s %s: %d detections, error of none_%s %.2e, of the head %.2e, E32 %.2e, bound %.2e, |none - head| %.2e'
              % (mode, k, n_det, k, e_mine, e_head, bnd[k][0], bnd[k][1], np.abs(mine - head).max()))
        assert np.isfinite(mine).all() and not got['none_' + k].cpu().numpy()[~live].any()
        if mode == 'float32':
            assert e_mine <= bnd[k][1] and np.abs(mine - head).max() <= 2 * bnd[k][1], k
    sure = ref['margin'] >= 2 * bnd['logits'][1]
    print('end to end %s class: %.2f %% of %d rows excluded' % (mode, 100 * (1 - sure.mean()), n_det))
    assert 1 - sure.mean() <= 0.01 and np.array_equal(got['none_class'].cpu().numpy()[live][sure], ref['class'][sure])
    assert bool((got['none_class'].cpu()[torch.from_numpy(~live)] == -1).all())
    r_ref = R.score(rows, slots, W, bias, A, method='react', c=np.float32(react.c))
    r_bnd = R.bounds(r_ref, R.score(rows, slots, W, bias, A, method='react', c=np.float32(react.c), dtype=np.float32))
    e_r = np.abs(got['react_energy'].cpu().numpy()[live] - r_ref['energy']).max()
    print('end to end %s react_energy: error %.2e, bound %.2e, c %.6g' % (mode, e_r, r_bnd['energy'][1], react.c))
    assert e_r <= r_bnd['energy'][1]
    # two sub-batch streams: the same keys, bitwise
    two = DetBenchPredict(model, streams=2, feature_ood=[none, react]).to(DEV)
    det2 = two(x)
    torch.cuda.synchronize()
    assert torch.equal(det2, det0)
    for k in none.KEYS + react.KEYS + ('energy', 'max_logit', 'anchor_index'):
        assert torch.equal(two.last_ood[k], bench.last_ood[k]), k
    # toggling the flag off again rebuilds the plan without the buffer
    model.keep_class_tower = False
    cls2, _ = model(x)
    assert model._engine.cls_tower is None and all(torch.equal(a, b) for a, b in zip(cls0, cls2))
