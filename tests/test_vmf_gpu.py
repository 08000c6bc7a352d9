"""ood_vmf.VMFHead / VMFFeatureOOD (csrc/vmf.hip) against the numpy restatement of tests/_vmf_ref.py.

Inputs (`_vmf_ref.inputs`): a seeded [B = 2, P, d] embedding (class directions plus noise, row norms in [0.5, 3]) and dense labels
with a chosen number of entries in [0, C), the rest from (-1, -2, C, C + 5); no network except where a test says so.

Bounds.  The partition function: 2^-30 relative, against max(1, |log Z|) for log Z and against A for A - the float32 logits these
values feed (2^-24) with a margin of 64 - on d in {2, 3, 16, 64, 255, 256} x kappa in {2^-7, 1, 10, 100, 1000, 8192}, at the
concentrations the device itself returns (kappa = float32(exp(theta)) may differ from numpy's by one float32 place: asserted).
Loss, dU, d theta and mean mu_y . r: within 4 E32 + 1e-7 max |value| of the float64 restatement, per key and case; E32 is the float32
restatement's own error on the same inputs, table and prototypes (the loss and the mean from their per-row terms).  The counts are
exact.  The prototype update is float32 with one rounding per operation and a stated order of the norm's sum, so it is compared bit
for bit.  Every case prints E32, the device error and the bound before it asserts."""
import functools

import numpy as np
import pytest
import torch

import _vmf_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
REL = 2.0 ** -30


def _head(C, A, d, theta=None, limit=None, ema=0.95):
    from ood_object_detection_amd.ood_vmf import VMFHead
    head = VMFHead(64, C, A, dim=d, ema=ema, ema_rows_per_class=limit).to(DEV)
    if theta is not None:
        with torch.no_grad():
            head.log_kappa.copy_(torch.from_numpy(np.asarray(theta, np.float32)))
    return head


def _theta(C):
    theta = np.log(np.random.RandomState(C).uniform(2.0, 40.0, C)).astype(np.float32)
    if C > 2:
        theta[1] = 20.0                                          # beyond the clamp: the flag is set, the gradient is zero
    return theta


def _table(head):
    """the device's own table as the restatement's `part`"""
    from ood_object_detection_amd.ood_vmf import partition
    p = partition(head.log_kappa, head.dim)
    return {'kappa': p['kappa'].cpu().numpy(), 'logz32': p['logz'].cpu().numpy(), 'logz': p['logz64'].cpu().numpy(),
            'ratio': p['ratio'].cpu().numpy(), 'clamped': p['clamped'].cpu().numpy().astype(bool)}


def _run(head, U, labels, update=True, upstream=None):
    """-> dict of device results: loss, dU, dtheta, stats"""
    leaf = torch.from_numpy(U.copy()).to(DEV).requires_grad_()
    head.log_kappa.grad = None
    loss, stats = head.loss(leaf, torch.from_numpy(labels.copy()).to(DEV), update=update)
    (loss if upstream is None else loss * upstream).backward()
    return dict(stats, loss=loss.detach(), dU=leaf.grad, dtheta=head.log_kappa.grad.clone())


def _eq(a, b):
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


@functools.lru_cache(maxsize=None)
def _inputs(P, d, A, C, n, nan=False):
    U, labels = R.inputs(2, P, d, A, C, n)
    if nan:
        U[0, 0, d // 2], labels[0, 0] = np.nan, 0               # a counted anchor on a row that holds a NaN
        U[1, 1, 0], labels[1, A] = np.inf, C - 1
    U.setflags(write=False)
    labels.setflags(write=False)
    return U, labels


def _check(got, ref, f32, name):
    bnd = R.bounds(ref, f32)
    for k, dev in (('loss', got['loss']), ('dU', got['dU']), ('dtheta', got['dtheta']), ('mean_dot', got['mean_cosine'])):
        val = dev.double().cpu().numpy().reshape(np.shape(ref[k]))
        err = float(np.abs(val - ref[k]).max()) if val.size else 0.0
        e32, b = bnd[k]
        print('%s %s: max |value| %.3g, device error %.2e, E32 %.2e, bound %.2e' % (name, k, float(np.abs(ref[k]).max()), err, e32, b))
        assert err <= b, (name, k, err, b)
    assert [int(got[k]) for k in ('m', 'skipped', 'valid_classes')] == [ref['m'], ref['skipped'], ref['valid_classes']], name
    assert abs(float(got['mean_kappa']) - ref['mean_kappa']) <= 1e-12 * ref['mean_kappa'] and float(got['max_kappa']) == ref['max_kappa']
    assert abs(float(got['loss64']) - float(ref['loss'])) <= bnd['loss'][1]


# ---- the partition function ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', [2, 3, 16, 64, 255, 256])
def test_partition_against_the_restatement(d):
    kap = np.array([2.0 ** -7, 1, 10, 100, 1000, 8192], np.float64)
    theta = np.log(kap).astype(np.float32)
    got = _table(_head(len(theta), 1, d, theta))
    ref = R.partition(theta, d)
    assert np.abs(got['kappa'].view(np.int32) - ref['kappa'].view(np.int32)).max() <= 1 and not got['clamped'].any()
    at = R.from_kappa(got['kappa'], d)
    ez = np.abs(got['logz'] - at['logz']) / np.maximum(1.0, np.abs(at['logz']))
    ea = np.abs(got['ratio'] - at['ratio']) / at['ratio']
    for k, a, b in zip(got['kappa'], ez, ea):
        print('d %3d kappa %9.4f: relative error of log Z %.1e, of A %.1e (bound %.1e)' % (d, k, a, b, REL))
    assert ez.max() <= REL and ea.max() <= REL
    assert np.array_equal(got['logz32'], got['logz'].astype(np.float32))


def test_partition_outside_the_clamp():
    theta = np.array([-100.0, 100.0, np.nan, R.THETA_LO, R.THETA_HI, 1.0], np.float32)
    got = _table(_head(6, 1, 64, theta))
    assert list(got['clamped']) == [True, True, True, False, False, False]
    assert np.abs(got['kappa'][:5] / np.array([2.0 ** -7, 8192, 2.0 ** -7, 2.0 ** -7, 8192]) - 1).max() <= 1e-6
    U, labels = _inputs(30, 64, 3, 6, 60)
    head = _head(6, 3, 64, theta)
    out = _run(head, U, labels)
    assert not out['dtheta'][:3].any() and out['dtheta'][3:].any() and torch.isfinite(out['dtheta']).all()


# ---- loss, dU, d theta, statistics ---------------------------------------------------------------------------------------------------
CASES = ([(40, d, 3, 7, 100, False) for d in (2, 16, 63, 64, 65, 256)] +           # the lane slice at 64 and the widest row
         [(30 * (10 - A), 16, A, C, 120, False) for A, C in ((9, 1), (9, 2), (1, 64), (9, 65), (9, 90), (9, 1024))] +      # no row for most classes
         [(1100, 8, 2, 3, n, False) for n in (0, 1, 63, 64, 65, 2047, 2048, 2049)] +  # the wave round and the 2048-entry tile
         [(40, 16, 9, 7, 300, True), (12, 16, 1, 5, 24, False)])                      # a NaN row; every entry counted


@pytest.mark.parametrize('P,d,A,C,n,nan', CASES)
def test_loss_and_gradients_against_the_restatement(P, d, A, C, n, nan):
    U, labels = _inputs(P, d, A, C, n, nan)
    head = _head(C, A, d, _theta(C))
    got = _run(head, U, labels)
    part = _table(head)
    proto, valid = head.prototypes.cpu().numpy(), head.valid.cpu().numpy().astype(bool)
    p_ref, v_ref = R.update(U, labels, A, np.zeros((C, d), np.float32), np.zeros(C, bool))
    assert np.array_equal(proto.view(np.uint32), p_ref.view(np.uint32)) and np.array_equal(valid, v_ref)
    ref, f32 = R.forward(U, labels, A, proto, valid, part), R.forward(U, labels, A, proto, valid, part, np.float32)
    name = 'P %d d %d A %d C %d counted %d' % (P, d, A, C, n)
    _check(got, ref, f32, name)
    assert (ref['skipped'] >= 2) if nan else (ref['m'] == n and ref['skipped'] == 0)
    counted = np.zeros(2 * P, bool)
    counted[ref['idx'] // A] = True
    assert not got['dU'].cpu().numpy().reshape(2 * P, d)[~counted].any(), name       # zeros for every other cell
    if C > 2:
        assert float(got['dtheta'][1]) == 0.0
    if n > 2 * P:
        assert len(set(ref['idx'] // A)) < ref['m']                                   # several anchors of one cell
    # labels as int32 and float32 read the same; an upstream gradient scales both gradients
    head2 = _head(C, A, d, _theta(C))
    leaf = torch.from_numpy(U.copy()).to(DEV).requires_grad_()
    loss, _ = head2.loss(leaf, torch.from_numpy(labels.astype(np.float32 if d % 2 else np.int32)).to(DEV))
    (loss * 0.5).backward()
    assert torch.equal(loss.detach(), got['loss']) and torch.equal(leaf.grad, got['dU'] * 0.5)
    assert torch.equal(head2.log_kappa.grad, got['dtheta'] * 0.5)


def test_invalid_classes_never_enter_a_softmax():
    from ood_object_detection_amd.ood_vmf import _score_embeddings
    P, d, A, C = 30, 16, 9, 90
    U, labels = _inputs(P, d, A, C, 60)
    head = _head(C, A, d, _theta(C))
    a = _run(head, U, labels)
    valid = head.valid.bool()
    assert 0 < int(valid.sum()) < C
    s0 = _score_embeddings(head, torch.from_numpy(U.copy()).to(DEV))[0]
    with torch.no_grad():
        head.prototypes[~valid] = float('nan')                  # what an invalid class holds cannot matter
        head.log_kappa[~valid] = 5.0
    b = _run(head, U, labels, update=False)
    # without the update the same prototypes give the same loss and gradients (kappa of the invalid classes moved: their statistics)
    for k in ('loss', 'dU', 'm', 'skipped', 'valid_classes', 'mean_cosine'):
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(a['dtheta'][valid], b['dtheta'][valid]) and not b['dtheta'][~valid].any()
    s1 = _score_embeddings(head, torch.from_numpy(U.copy()).to(DEV))[0]
    assert _eq(s0, s1) and bool(valid[s1['vmf_class']].all())
    # a label whose class has no prototype does not count when the update is off
    fresh = _head(C, A, d, _theta(C))
    out = _run(fresh, U, labels, update=False)
    assert int(out['m']) == 0 and float(out['loss']) == 0.0 and not out['dU'].any() and not out['dtheta'].any()
    assert not fresh.valid.any() and not fresh.prototypes.any()


# ---- the prototype update -------------------------------------------------------------------------------------------------------------
def _update(head, U, labels):
    from ood_object_detection_amd.ood_vmf import update_prototypes
    update_prototypes(torch.from_numpy(np.array(U)).to(DEV), torch.from_numpy(np.array(labels)).to(DEV), head.A,
                      head.prototypes, head.valid, head.ema, head.ema_rows_per_class)
    return head.prototypes.cpu().numpy(), head.valid.cpu().numpy().astype(bool)


def test_update_of_2049_rows_of_one_class_bit_for_bit():
    P, d, A, C = 1100, 8, 2, 3
    U, _ = _inputs(P, d, A, C, 0)
    labels = np.full((2, A * P), -1, np.int64)
    labels.reshape(-1)[np.random.RandomState(1).choice(2 * A * P, 2049, replace=False)] = 1
    got = _update(_head(C, A, d), U, labels)
    ref = R.update(U, labels, A, np.zeros((C, d), np.float32), np.zeros(C, bool))
    assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32)) and list(got[1]) == [False, True, False]


@pytest.mark.parametrize('limit', [1, 64, 65])
def test_update_rows_per_class(limit):
    P, d, A, C = 40, 16, 9, 3
    U, labels = _inputs(P, d, A, C, 400)
    got = _update(_head(C, A, d, limit=limit, ema=0.9), U, labels)
    ref = R.update(U, labels, A, np.zeros((C, d), np.float32), np.zeros(C, bool), 0.9, limit)
    assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32)) and np.array_equal(got[1], ref[1]) and ref[1].all()
    assert (np.bincount(labels.reshape(-1)[(labels.reshape(-1) >= 0) & (labels.reshape(-1) < C)], minlength=C) > 65).all()


def test_update_in_two_calls_equals_one_call():
    P, d, A, C = 40, 64, 9, 7
    U, labels = _inputs(P, d, A, C, 300)
    one = _update(_head(C, A, d), U, labels)
    head = _head(C, A, d)
    _update(head, U[:1], labels[:1])
    two = _update(head, U[1:], labels[1:])
    assert np.array_equal(one[0].view(np.uint32), two[0].view(np.uint32)) and np.array_equal(one[1], two[1])
    ref = R.update(U, labels, A, np.zeros((C, d), np.float32), np.zeros(C, bool))
    assert np.array_equal(one[0].view(np.uint32), ref[0].view(np.uint32))


# ---- scores --------------------------------------------------------------------------------------------------------------------------
def _trained(P, d, A, C, n):
    U, labels = _inputs(P, d, A, C, n)
    head = _head(C, A, d, _theta(C))
    _update(head, U, labels)
    return head, U, labels


@pytest.mark.parametrize('P,d,A,C', [(40, 16, 9, 7), (30, 65, 3, 90), (100, 256, 1, 130)])
def test_scores_against_the_restatement_and_however_grouped(P, d, A, C):
    from ood_object_detection_amd.ood_vmf import _score_embeddings
    head, U, _ = _trained(P, d, A, C, 150)
    Ut = torch.from_numpy(U.copy()).to(DEV)
    cells, unit = _score_embeddings(head, Ut, want_rows=True)
    part, proto, valid = _table(head), head.prototypes.cpu().numpy(), head.valid.cpu().numpy().astype(bool)
    ref, f32 = (R.score(U.reshape(2 * P, d), proto, valid, part, dt) for dt in (np.float64, np.float32))
    for k in ('vmf', 'vmf_cosine'):
        err = float(np.abs(cells[k].double().cpu().numpy().reshape(-1) - ref[k]).max())
        e32, b = R.bound(ref[k], f32[k])
        print('P %d d %d C %d %s: max |value| %.3g, device error %.2e, E32 %.2e, bound %.2e' % (P, d, C, k, np.abs(ref[k]).max(), err, e32, b))
        assert err <= b, k
    sure = ref['margin'] > 2 * R.bound(ref['vmf'], f32['vmf'])[1]
    assert sure.mean() > 0.9 and np.array_equal(cells['vmf_class'].cpu().numpy().reshape(-1)[sure], ref['vmf_class'][sure])
    assert np.abs(unit.double().cpu().numpy().reshape(2 * P, d) - ref['unit']).max() <= 1e-6
    # one image of 2 P cells, and the cells in another order: the same bits per row
    flat = _score_embeddings(head, Ut.reshape(1, 2 * P, d))[0]
    assert all(torch.equal(flat[k].reshape(2, P), cells[k]) for k in cells)
    perm = torch.randperm(P, generator=torch.Generator().manual_seed(3)).to(DEV)
    moved = _score_embeddings(head, Ut[:, perm].contiguous())[0]
    assert all(torch.equal(moved[k], cells[k][:, perm]) for k in cells)
    # selected anchors: the cell's scores; -1 / 0 beyond count and for an anchor outside [0, A P)
    K = 37
    anchor = torch.randint(0, A * P, (2, K), generator=torch.Generator().manual_seed(5)).to(DEV)
    anchor[0, 3], anchor[1, 5] = -1, A * P
    count = torch.tensor([K - 4, K], dtype=torch.int32, device=DEV)
    sel, rows = _score_embeddings(head, Ut, anchor, count, want_rows=True)
    ok = (torch.arange(K, device=DEV)[None] < count[:, None]) & (anchor >= 0) & (anchor < A * P)
    cell = torch.where(ok, anchor // A, torch.zeros_like(anchor))
    for k in cells:
        want = torch.where(ok, torch.gather(cells[k], 1, cell), torch.full_like(cells[k][:, :1], -1 if k == 'vmf_class' else 0))
        assert torch.equal(sel[k], want), k
    assert torch.equal(rows, torch.where(ok[:, :, None], torch.gather(unit, 1, cell[:, :, None].expand(2, K, d)), torch.zeros_like(rows)))
    # the same rows gathered beforehand (the form the scorer uses behind the MLP): bit for bit, with no MLP in between
    picked = torch.gather(Ut, 1, cell[:, :, None].expand(2, K, d)).contiguous()
    gsel, grows = _score_embeddings(head, picked, anchor, count, want_rows=True, gathered_cells=P)
    assert all(torch.equal(gsel[k], sel[k]) for k in sel) and torch.equal(grows, rows)


def test_score_ties_go_to_the_lowest_class_and_no_valid_class():
    from ood_object_detection_amd.ood_vmf import _score_embeddings
    head, U, _ = _trained(40, 16, 9, 7, 150)
    assert bool(head.valid.all())
    with torch.no_grad():
        head.prototypes[5] = head.prototypes[2]
        head.log_kappa[5] = head.log_kappa[2]
    s = _score_embeddings(head, torch.from_numpy(U.copy()).to(DEV))[0]
    assert int((s['vmf_class'] == 2).sum()) > 0 and int((s['vmf_class'] == 5).sum()) == 0
    empty = _score_embeddings(_head(7, 9, 16), torch.from_numpy(U.copy()).to(DEV))[0]
    assert not empty['vmf'].any() and bool((empty['vmf_class'] == -1).all()) and not empty['vmf_cosine'].any()


def _levels(B, shapes, F, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, h, w, F, generator=g).to(DEV).to(dtype).permute(0, 3, 1, 2) for h, w in shapes]


def test_scorer_on_a_tower_float32_and_bfloat16():
    """through gather and the MLP: a bfloat16 tower scores like its float32 widening, bit for bit; score() at gathered anchors agrees
    with score_cells() at those cells (the GEMM's dispatch form depends on the number of rows, so within float32 rounding of the
    embedding: 1e-5 of the logit scale)"""
    from ood_object_detection_amd.ood_features import KNNFeatureOOD
    from ood_object_detection_amd.ood_vmf import VMFFeatureOOD
    shapes, A, C, d = ((8, 8), (4, 4), (2, 2), (1, 1)), 9, 5, 64
    P = sum(h * w for h, w in shapes)
    head = _head(C, A, d)
    lv16 = _levels(2, shapes, 64, torch.bfloat16)
    lv32 = [t.float() for t in lv16]
    labels = torch.randint(-2, C, (2, A * P), generator=torch.Generator().manual_seed(1)).to(DEV)
    loss, stats = head(lv32, labels)
    assert int(stats['m']) > 0 and bool(head.valid.all()) and bool(torch.isfinite(loss))
    loss.backward()
    assert all(p.grad is not None and bool(p.grad.abs().sum() > 0) for p in head.parameters())
    scorer = VMFFeatureOOD(head)
    c32, c16 = scorer.score_cells(lv32), scorer.score_cells(lv16)
    assert _eq(c32, c16) and tuple(c32['vmf'].shape) == (2, P) and c32['vmf_class'].dtype == torch.int64
    K = 21
    anchor = torch.randint(0, A * P, (2, K), generator=torch.Generator().manual_seed(2)).to(DEV)
    count = torch.tensor([K, K - 5], device=DEV)
    s32, s16 = scorer.score(lv32, anchor, count), scorer.score(lv16, anchor, count)
    assert _eq(s32, s16)
    ok = torch.arange(K, device=DEV)[None] < count[:, None]
    scale = float(c32['vmf'].abs().max())
    for k in ('vmf', 'vmf_cosine'):
        want = torch.where(ok, torch.gather(c32[k], 1, anchor // A), torch.zeros_like(s32[k]))
        assert float((s32[k] - want).abs().max()) <= 1e-5 * max(scale, 1.0), k
    assert bool((s32['vmf_class'][~ok] == -1).all())
    # SIREN's k-NN variant: at dim = 64 the unit embeddings are a feature tensor of KNNFeatureOOD
    emb = scorer.embeddings(lv32)
    assert tuple(emb.shape) == (2, P, d) and float((emb.norm(dim=2) - 1).abs().max()) <= 1e-5
    knn = KNNFeatureOOD(64, A, capacity=4096, k=3)
    knn.add(emb)
    knn.fit()
    out = knn.score(emb, anchor, count)
    assert tuple(out['knn'].shape) == (2, K) and bool(torch.isfinite(out['knn']).all())
    sel = scorer.embeddings(lv32, anchor, count)
    assert tuple(sel.shape) == (2, K, d) and not sel[~ok].any()


# ---- determinism and capture -------------------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical():
    P, d, A, C = 40, 64, 9, 90
    U, labels = _inputs(P, d, A, C, 300)
    h1, h2 = _head(C, A, d, _theta(C)), _head(C, A, d, _theta(C))
    a, b = _run(h1, U, labels), _run(h2, U, labels)
    assert _eq(a, b) and torch.equal(h1.prototypes, h2.prototypes) and torch.equal(h1.valid, h2.valid)


def test_graph_replay_of_update_and_loss():
    P, d, A, C = 40, 64, 9, 90
    U, labels = _inputs(P, d, A, C, 300)
    head = _head(C, A, d, _theta(C))
    eager = _run(head, U, labels)
    p_eager, v_eager = head.prototypes.clone(), head.valid.clone()
    s_u = torch.zeros(2, P, d, device=DEV).requires_grad_()
    s_l = torch.full((2, A * P), -1, dtype=torch.int64, device=DEV)
    s_u.grad = torch.zeros_like(s_u)
    head.log_kappa.grad = torch.zeros_like(head.log_kappa)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            s_u.grad.zero_()
            head.log_kappa.grad.zero_()
            loss, stats = head.loss(s_u, s_l)
            loss.backward()
    torch.cuda.current_stream(DEV).wait_stream(side)
    with torch.no_grad():
        s_u.copy_(torch.from_numpy(U.copy()))
    s_l.copy_(torch.from_numpy(labels.copy()))
    for _ in range(2):
        head.prototypes.zero_()
        head.valid.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss.detach(), eager['loss']) and all(torch.equal(stats[k], eager[k]) for k in stats)
        assert torch.equal(s_u.grad, eager['dU']) and torch.equal(head.log_kappa.grad, eager['dtheta'])
        assert torch.equal(head.prototypes, p_eager) and torch.equal(head.valid, v_eager)
