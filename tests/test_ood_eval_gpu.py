"""ood.detection_metrics / ood.OODEvaluator (csrc/ood_eval.hip) against the float64 restatement of tests/_ood_eval_ref.py.

Integers (pairs_gt, pairs_eq, tp, fp, n_in, n_ood) and the threshold are exact, sorted_scores() is bit-equal to np.sort of the
canonicalised input, auroc is within 1e-12 (it is formed from equal integers), aupr_in / aupr_out within (G + 8) * 2^-53, G the
number of distinct values on the summed side (_ood_eval_ref.aupr_bound: three roundings per term, and sums of non-negative terms
that stay <= 1).  Every case prints its deviation before it asserts."""
import numpy as np
import pytest
import torch

import _ood_eval_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
_REF = {}


def _tile():
    from ood_object_detection_amd import _lib
    return _lib.load().effdet_ood_eval_sort_tile()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _compare(got, ref, name):
    e_in, e_out = abs(got['aupr_in'] - ref['aupr_in']), abs(got['aupr_out'] - ref['aupr_out'])
    print('%s: P %d N %d auroc %.6f aupr_in %.6f aupr_out %.6f fpr %.6f; aupr deviation %.2e / %.2e (bounds %.2e / %.2e)'
          % (name, got['n_in'], got['n_ood'], got['auroc'], got['aupr_in'], got['aupr_out'], got['fpr_at_tpr'], e_in, e_out,
             R.aupr_bound(ref['groups_in']), R.aupr_bound(ref['groups_out'])))
    for k in R.INT_KEYS + ('threshold',):
        assert got[k] == ref[k], (name, k, got[k], ref[k])
    assert abs(got['auroc'] - ref['auroc']) <= 1e-12, name
    assert got['fpr_at_tpr'] == ref['fpr_at_tpr'] and got['tpr'] == ref['tpr'], name
    assert e_in <= R.aupr_bound(ref['groups_in']), (name, e_in)
    assert e_out <= R.aupr_bound(ref['groups_out']), (name, e_out)


def _check(pos, neg, level=0.95, name='', slack=0):
    """one-shot through an evaluator (so that the sorted arrays can be read), against the restatement"""
    from ood_object_detection_amd import ood
    pos, neg = np.asarray(pos, np.float32).reshape(-1), np.asarray(neg, np.float32).reshape(-1)
    ev = ood.OODEvaluator(pos.size + slack, neg.size + slack, DEV)
    ev.add(_dev(pos), False)
    ev.add(_dev(neg), True)
    got, ref = ev.evaluate(level), R.metrics(pos, neg, level)
    _compare(got, ref, name)
    for x, s in zip((pos, neg), ev.sorted_scores()):
        assert np.array_equal(s.cpu().numpy().view(np.uint32), np.sort(R.canonical(x)).view(np.uint32)), (name, 'sorted_scores')
    return got, ev


@pytest.mark.parametrize('pos,neg,gt,eq', [([1.0], [0.5], 1, 0), ([0.5], [1.0], 0, 0), ([0.5], [0.5], 0, 1), ([-0.0], [0.0], 0, 1)])
def test_one_score_a_side(pos, neg, gt, eq):
    got, _ = _check(pos, neg, name='1 x 1')
    assert (got['pairs_gt'], got['pairs_eq']) == (gt, eq) and got['auroc'] == gt + 0.5 * eq


def test_one_against_five():
    rs = np.random.RandomState(1)
    _check([0.3], rs.normal(0, 1, 5), name='1 x 5')
    _check(rs.normal(0, 1, 5), [0.3], name='5 x 1')
    from ood_object_detection_amd import ood
    got = ood.detection_metrics(_dev([0.1, 0.7, 0.7, -2.0, 0.3]), _dev([0.3]))
    _compare(got, R.metrics([0.1, 0.7, 0.7, -2.0, 0.3], [0.3]), 'detection_metrics 5 x 1')


@pytest.mark.parametrize('shift', [0.0, 0.4])
def test_tile_boundaries(shift):
    T, rs = _tile(), np.random.RandomState(2)
    sizes = [T - 1, T, T + 1, 3 * T + 17]
    for p, n in zip(sizes, sizes[1:] + sizes[:1]):                      # paired unequally
        _check(rs.normal(0, 1, p), rs.normal(0, 1, n) - shift, name='tiles %d x %d, shift %.1f' % (p, n, shift), slack=p % 3)


def test_heavy_ties():
    T, rs = _tile(), np.random.RandomState(3)
    _check(np.round(rs.normal(0.4, 1, 2 * T + 5) * 2) / 2, np.round(rs.normal(0, 1, T + 9) * 2) / 2, name='halves')
    _check(np.round(rs.normal(0, 1, 500) * 2) / 2, np.round(rs.normal(0, 1, 3 * T + 17) * 2) / 2, level=0.5, name='halves, level 0.5')


def test_all_equal():
    T = _tile()
    got, _ = _check(np.full(3 * T + 17, 0.25), np.full(2 * T + 5, 0.25), name='all equal')
    assert got['pairs_eq'] == (3 * T + 17) * (2 * T + 5) and got['pairs_gt'] == 0 and got['auroc'] == 0.5
    assert got['tp'] == 3 * T + 17 and got['fp'] == 2 * T + 5


def _byte_patterns(b, sign, rs, n):
    """float32 values in which only byte b of the bit pattern varies (finite exponents), with the given sign"""
    if b == 3:
        x = (rs.randint(0, 127, n).astype(np.uint32) << np.uint32(24)) | np.uint32(0x00400000)
    else:
        x = (np.uint32(0x3F000000) & ~np.uint32(0xFF << (8 * b))) | (rs.randint(0, 256, n).astype(np.uint32) << np.uint32(8 * b))
    return (x | np.uint32(sign << 31)).view(np.float32)


@pytest.mark.parametrize('b', [0, 1, 2, 3])
def test_digit_isolation(b):
    T, rs = _tile(), np.random.RandomState(4 + b)
    pos = np.concatenate([_byte_patterns(b, 0, rs, T + 3), _byte_patterns(b, 1, rs, T // 2)])
    neg = np.concatenate([_byte_patterns(b, 1, rs, T + 1), _byte_patterns(b, 0, rs, 777)])
    _check(rs.permutation(pos), rs.permutation(neg), name='only byte %d varies' % b)


def test_special_values():
    fmax = np.finfo(np.float32).max
    sp = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1e-39, -1e-39, fmax, -fmax, 1.0, -1.0, 0.0, -0.0], np.float32)
    rs = np.random.RandomState(5)
    _check(sp, sp[::-1][:9], level=1.0, name='special values')
    _check(np.concatenate([sp, rs.normal(0, 1, 300).astype(np.float32)]), np.concatenate([rs.normal(0, 1e-38, 200).astype(np.float32), sp]),
           name='special values among others')


def test_extremes():
    rs = np.random.RandomState(6)
    hi, lo = rs.uniform(1, 2, 1500), rs.uniform(-2, -1, 700)
    got, _ = _check(hi, lo, name='separated')
    assert got['auroc'] == 1.0 and got['fpr_at_tpr'] == 0.0
    got, _ = _check(lo, hi, name='reversed')
    assert got['auroc'] == 0.0 and got['fpr_at_tpr'] == 1.0
    x, y = rs.normal(0.3, 1, 1001), rs.normal(0, 1, 777)
    got, _ = _check(x, y, level=1.0, name='level 1')
    assert got['tp'] == 1001 and got['threshold'] == float(np.float32(x).min())
    got, _ = _check(x, y, level=1e-9, name='level 1e-9')
    assert got['tp'] == 1 and got['threshold'] == float(np.float32(x).max())


@pytest.mark.parametrize('rounded', [True, False])
def test_size(rounded):
    rs = np.random.RandomState(7)
    pos, neg = rs.normal(0.4, 1, 1 << 20).astype(np.float32), rs.normal(0, 1, 1 << 19).astype(np.float32)
    if rounded:
        pos, neg = np.round(pos, 3), np.round(neg, 3)
    _check(pos, neg, name='2^20 x 2^19, %s' % ('rounded to 1e-3' if rounded else 'continuous'))


def _raw(ev):
    return ev._result.cpu().numpy().tobytes()


def test_reproducible_bits():
    from ood_object_detection_amd import ood
    T, rs = _tile(), np.random.RandomState(8)
    pos, neg = np.round(rs.normal(0.4, 1, 5 * T + 3), 2).astype(np.float32), np.round(rs.normal(0, 1, 2 * T + 11), 2).astype(np.float32)
    blocks = []
    for perm in (False, True):
        ev = ood.OODEvaluator(pos.size, neg.size, DEV)
        ev.add(_dev(rs.permutation(pos) if perm else pos), False)
        ev.add(_dev(rs.permutation(neg) if perm else neg), True)
        ev.evaluate()
        blocks.append(_raw(ev))
        ev.evaluate()
        blocks.append(_raw(ev))
    assert all(b == blocks[0] for b in blocks)


def test_agrees_with_pair_counting_auroc():
    from ood_object_detection_amd import ood
    rs = np.random.RandomState(9)
    pos, neg = _dev(np.round(rs.normal(0.4, 1, 3000), 2)), _dev(np.round(rs.normal(0, 1, 2500), 2))
    got = ood.detection_metrics(pos, neg)
    assert abs(got['auroc'] - ood.auroc(pos, neg)) <= 1e-12


def _accumulation_case(rs, B=5, K=100):
    full = rs.normal(0, 1, (B, 3 * K)).astype(np.float32)
    det = rs.uniform(0, 1, (B, K, 6)).astype(np.float32)
    count = np.array([0, K, 7, K - 1, 1][:B], np.int32)
    return full, det, count


def test_accumulation_equals_one_shot():
    from ood_object_detection_amd import ood
    rs = np.random.RandomState(10)
    B, K = 5, 100
    full, det, count = _accumulation_case(rs, B, K)
    g_full, g_det, g_count = _dev(full), _dev(det), torch.from_numpy(count).to(DEV)
    in_count = np.arange(K)[None, :] < count[:, None]
    extra = rs.normal(0.2, 1, 333).astype(np.float32)
    block = rs.normal(0, 1, (3, 41)).astype(np.float32)
    ev = ood.OODEvaluator(4096, 4096, DEV)
    ev.add_detections(g_full[:, 0:K], g_count, False, det_scores=g_det[:, :, 4], min_score=0.3, negate=True)     # contiguous rows, pitch 3K
    ev.add_detections(g_full[:, K::2], g_count.long(), True)                                                     # element stride 2, int64 counts
    ev.add(_dev(extra), False)
    ev.add(_dev(block), True)
    ev.add_detections(g_full[:, 0:K], None, True, negate=True)                                                   # no counts: all K
    pos = np.concatenate([-full[:, 0:K][in_count & (det[:, :, 4] >= 0.3)], extra])
    neg = np.concatenate([full[:, K::2][in_count], block.reshape(-1), -full[:, 0:K].reshape(-1)])
    got = ev.evaluate()
    assert np.array_equal(ev._bufs[0][:pos.size].cpu().numpy(), pos) and np.array_equal(ev._bufs[1][:neg.size].cpu().numpy(), neg), '(b, j) order'
    _compare(got, R.metrics(pos, neg), 'five ragged appends')
    one = ood.detection_metrics(_dev(pos), _dev(neg))
    assert one == got
    ev.clear()
    ev.add(_dev(extra), False)
    ev.add(_dev(block), True)
    _compare(ev.evaluate(), R.metrics(extra, block), 'after clear()')


def test_capacity_overflow_is_reported_and_bounded():
    from ood_object_detection_amd import ood
    rs = np.random.RandomState(11)
    T = _tile()
    n, sentinel = T + 40, -12345.5
    store = torch.full((n - 1 + 4096,), sentinel, dtype=torch.float32, device=DEV)
    other = torch.empty(64, dtype=torch.float32, device=DEV)
    ev = ood.OODEvaluator(n - 1, 64, DEV, storage=(store[:n - 1], other))
    x = rs.normal(0, 1, n).astype(np.float32)
    ev.add(_dev(x[:T]), False)
    ev.add(_dev(x[T:]), False)
    ev.add(_dev(x[:10]), True)
    with pytest.raises(ValueError, match='in-distribution capacity overflowed'):
        ev.evaluate()
    assert bool((store[n - 1:] == sentinel).all()), 'a write beyond the capacity'
    assert np.array_equal(store[:n - 1].cpu().numpy(), x[:n - 1])
    ev2 = ood.OODEvaluator(64, 9, DEV)
    ev2.add(_dev(x[:10]), False)
    ev2.add(_dev(x[:10]), True)
    with pytest.raises(ValueError, match='OOD capacity overflowed'):
        ev2.evaluate()


def test_nan_and_empty_side_are_reported():
    from ood_object_detection_amd import ood
    x = np.arange(100, dtype=np.float32)
    y = x.copy()
    y[37] = np.nan
    with pytest.raises(ValueError, match='NaN among the OOD'):
        ood.detection_metrics(_dev(x), _dev(y))
    with pytest.raises(ValueError, match='NaN among the in-distribution'):
        ood.detection_metrics(_dev(y), _dev(x))
    ev = ood.OODEvaluator(16, 16, DEV)
    ev.add(_dev(x[:5]), True)
    with pytest.raises(ValueError, match='in-distribution side is empty'):
        ev.evaluate()
    with pytest.raises(ValueError, match='OOD side is empty'):
        ood.detection_metrics(_dev(x), _dev(x[:0]))


def test_add_after_evaluate_keeps_the_earlier_scores():
    from ood_object_detection_amd import ood
    rs = np.random.RandomState(13)
    a, b, c = (rs.normal(m, 1, n).astype(np.float32) for m, n in ((0.3, 700), (0.0, 900), (0.5, 5000)))
    ev = ood.OODEvaluator(8192, 8192, DEV)
    ev.add(_dev(a), False)
    ev.add(_dev(b), True)
    _compare(ev.evaluate(), R.metrics(a, b), 'first evaluate')
    ev.add(_dev(c), False)
    _compare(ev.evaluate(0.9), R.metrics(np.concatenate([a, c]), b, 0.9), 'more scores, second evaluate')


def test_limits_are_refused_before_any_launch():
    from ood_object_detection_amd import _lib
    lib = _lib.load()
    x = torch.zeros(64, dtype=torch.float32, device=DEV)
    state, result = torch.zeros(4, dtype=torch.int32, device=DEV), torch.zeros(12, dtype=torch.int64, device=DEV)
    need = lib.effdet_ood_eval_workspace_bytes(64, 64)
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    big = (1 << 27) + 1
    assert lib.effdet_ood_eval_sort(st, x.data_ptr(), 64, x.data_ptr(), 64, state.data_ptr(), ws.data_ptr(), need - 1) == -22
    assert lib.effdet_ood_eval_sort(st, x.data_ptr(), big, x.data_ptr(), 64, state.data_ptr(), ws.data_ptr(), need) == -22
    assert lib.effdet_ood_eval_metrics(st, 64, 64, state.data_ptr(), ws.data_ptr(), need - 1, 0.95, result.data_ptr()) == -22
    assert lib.effdet_ood_eval_metrics(st, 64, big, state.data_ptr(), ws.data_ptr(), need, 0.95, result.data_ptr()) == -22
    assert lib.effdet_ood_eval_metrics(st, 64, 64, state.data_ptr(), ws.data_ptr(), need, 0.0, result.data_ptr()) == -22
    for cap, nbytes in ((big, need), (64, 1024)):
        assert lib.effdet_ood_eval_append(st, x.data_ptr(), 64, 1, 1, 64, None, 0, None, 0, 0, 0.0, 0, x.data_ptr(), cap,
                                          state.data_ptr(), ws.data_ptr(), nbytes) == -22
    torch.cuda.synchronize()
    assert int(state.abs().sum()) == 0 and int(result.abs().sum()) == 0


def test_graph_capture():
    """add_detections + sort + metrics in one captured graph on one stream (no parallel branches), replayed on new scores"""
    from ood_object_detection_amd import ood
    rs = np.random.RandomState(12)
    B, K = 4, 100
    batches = [(rs.normal(0.5, 1, (B, K)).astype(np.float32), rs.normal(0, 1, (B, K)).astype(np.float32),
                rs.randint(0, K + 1, B).astype(np.int32)) for _ in range(3)]
    e_in, e_ood = torch.zeros(B, K, device=DEV), torch.zeros(B, K, device=DEV)
    cnt = torch.zeros(B, dtype=torch.int32, device=DEV)

    def load(b):
        for dst, src in zip((e_in, e_ood, cnt), b):
            dst.copy_(torch.from_numpy(src))

    def step(ev):
        ev.add_detections(e_in, cnt, False, negate=True)
        ev.add_detections(e_ood, cnt, True, negate=True)
        ev.enqueue()

    ev = ood.OODEvaluator(3 * B * K, 3 * B * K, DEV)
    ev.clear()                                                          # allocates before the capture
    stream = torch.cuda.Stream(DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(stream):
        load(batches[0])
        step(ev)                                                        # warm-up on the capture stream
        ev.clear()
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            step(ev)
    torch.cuda.current_stream(DEV).wait_stream(stream)
    torch.cuda.synchronize()
    ev.clear()                                                          # the capture itself ran nothing
    eager = ood.OODEvaluator(3 * B * K, 3 * B * K, DEV)
    for i, b in enumerate(batches[1:]):
        load(b)
        graph.replay()
        step(eager)
        torch.cuda.synchronize()
        got, want = ev.result(), eager.result()
        assert got == want and _raw(ev) == _raw(eager), i
    pos =np.concatenate([-b[0][np.arange(K)[None, :] < b[2][:, None]] for b in batches[1:]])
    neg = np.concatenate([-b[1][np.arange(K)[None, :] < b[2][:, None]] for b in batches[1:]])
    _compare(got, R.metrics(pos, neg), 'two graph replays')
