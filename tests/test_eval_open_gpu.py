"""Open-set detection evaluation on the device (-m gpu): `OpenSetDetectionEvaluator`, `ood.relabel_unknown` and
`OODEvaluator.threshold_tensor` against the numpy restatement of tests/_eval_open_ref.py, against `DatasetDetectionEvaluator` with
one more class (bit for bit) and against themselves (runs, splits, a captured graph).

Integers, flag words and open words are compared EXACTLY; AP is compared bitwise with the closed-set evaluator (the same kernels on
the same entries) and within 1e-12 with the restatement (fewer than 1000 true positives a class: the bound derived in
tests/test_eval_scale_gpu.py).  No row is excluded anywhere."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _eval_open_ref as O
import _eval_scale_ref as R

DEV = 'cuda:0'
INVALID = 0x80000000


def _cats(C):
    return [{'id': i + 1, 'name': 'c%d' % i} for i in range(C)]


def _open(C, thresholds=(0.5,), **kw):
    from ood_object_detection_amd.effdet.evaluation import OpenSetDetectionEvaluator
    return OpenSetDetectionEvaluator(_cats(C), iou_thresholds=thresholds, device=DEV, **kw)


def _closed(C1, thresholds=(0.5,), **kw):
    from ood_object_detection_amd.effdet.evaluation import DatasetDetectionEvaluator
    return DatasetDetectionEvaluator(_cats(C1), iou_thresholds=thresholds, device=DEV, **kw)


def _dev(arrays):
    return [torch.from_numpy(a).to(DEV) for a in arrays]


def _u32(t):
    return t.cpu().numpy().astype(np.int64) & 0xFFFFFFFF


def _closed_words(T, C1):
    from ood_object_detection_amd.effdet.evaluation.dataset_evaluator import RESULT_HEAD
    return RESULT_HEAD + 2 * T * C1 + 2 * C1


def _assert_matches_ref(r, ref, name=''):
    for k in O.MATRICES + ('gt_count', 'gt_imgs', 'correct', 'a_ose'):
        assert np.array_equal(r[k], ref[k]), (name, k, r[k], ref[k])
    assert np.array_equal(np.isnan(r['ap']), np.isnan(ref['ap'])), name
    assert np.allclose(r['ap'], ref['ap'], rtol=0, atol=1e-12, equal_nan=True), name
    for k in ('wi', 'u_recall', 'u_precision', 'recall', 'precision', 'precision_at_recall'):
        assert np.array_equal(r[k], ref[k], equal_nan=True), (name, k, r[k], ref[k])           # the same float64 division of the same integers


# ------------------------------------------------------------------------------------------------ equivalence with the closed set
@pytest.mark.parametrize('T', [1, 10])
def test_without_unknowns_equals_the_closed_set_evaluator_bit_for_bit(T):
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'evaluation_scale.npz'))
    images, C = R.fixture_case(g, 'a')                                        # classes 0..C-1 with difficult flags; nothing of class C
    assert sum(int(im['gt_difficult'].sum()) for im in images) == 13
    thresholds = [round(0.5 + 0.05 * i, 2) for i in range(T)]
    packed = _dev(O.pack(images, 40, 5))
    ev, closed = _open(C, thresholds, capacity=4096), _closed(C + 1, thresholds, capacity=4096)
    flags, words = ev.add_batch(*packed)
    assert torch.equal(flags, closed.add_batch(*packed)) and not words.any()
    ev.enqueue()
    closed.enqueue()
    r, rc = ev.result(), closed.result()
    assert np.array_equal(r['block'][:_closed_words(T, C + 1)], rc['block']) and np.isfinite(rc['ap']).sum() >= 3 * T
    assert not r['open_total'].any() and not r['open_at'].any() and not r['a_ose'].any() and (r['wi'] == 0).all()
    assert np.array_equal(r['n_det'], O.evaluate(images, C, thresholds)['n_det'])
    # a loop can switch over: every key of the closed-set evaluator over the C known classes, with the same value
    from ood_object_detection_amd.effdet.evaluation import DatasetDetectionEvaluator, OpenSetDetectionEvaluator
    kw = dict(iou_thresholds=thresholds, capacity=4096, evaluate_corlocs=True, metric_prefix='val', device=DEV)
    a, b = DatasetDetectionEvaluator(_cats(C), **kw), OpenSetDetectionEvaluator(_cats(C), **kw)
    a.add_batch(*packed)
    b.add_batch(*packed)
    ma, mb = a.evaluate(), b.evaluate()
    assert 'val_Precision/meanCorLoc@0.5IOU' in ma and 'CorLoc@0.5IOU/c0' in ma and len(mb) > len(ma)
    for k, v in ma.items():
        assert np.array_equal(np.float64(mb[k]).view(np.int64), np.float64(v).view(np.int64)), k


def test_unknown_as_a_class_equals_the_closed_set_evaluator_bit_for_bit():
    C, M, thresholds = 5, 64, O.CASE_THRESHOLDS
    images = O.open_case(41, 6, 100, C, M, 20)
    packed = _dev(O.pack(images, 100, M))
    ev, closed = _open(C, thresholds, capacity=1024), _closed(C + 1, thresholds, capacity=1024)
    flags, words = ev.add_batch(*packed)
    assert torch.equal(flags, closed.add_batch(*packed)) and words.any()
    ev.enqueue()
    closed.enqueue()
    r, rc = ev.result(), closed.result()
    assert np.array_equal(r['block'][:_closed_words(3, C + 1)], rc['block'])
    assert rc['gt_count'][C] > 0 and 0 < rc['ap'][1, C] < 1 and r['tp'][1, C] > 0                 # the unknown column is alive
    cls, sc, fl, op = ev.sorted()
    ccls, csc, cfl = closed.sorted()
    assert np.array_equal(cls, ccls) and np.array_equal(sc.view(np.uint32), csc.view(np.uint32)) and np.array_equal(fl, cfl)
    assert len(op) == len(fl) and not op[cls == C].any()


# ------------------------------------------------------------------------------------------------ open words and counts
@pytest.mark.parametrize('M,n_unknown,max_det', [(1, 0, 100), (1, 1, 100), (64, 40, 100), (256, 1, 100), (256, 40, 300), (257, 257, 100),
                                                 (300, 257, 300), (300, 300, 100), (300, 0, 100)])
def test_open_words_and_counts_equal_the_restatement(M, n_unknown, max_det):
    C, B, thresholds, level = 5, 6, O.CASE_THRESHOLDS, 0.8
    images = O.open_case(100 + M + n_unknown, B, max_det - 3, C, M, n_unknown)
    ref = O.evaluate(images, C, thresholds, level)
    ev = _open(C, thresholds, recall_level=level, capacity=B * max_det)
    flags, words = ev.add_batch(*_dev(O.pack(images, max_det, M)))
    flags, words = _u32(flags), _u32(words)
    k = 0
    for i, im in enumerate(images):
        n = len(im['det_scores'])
        assert np.array_equal(flags[i, :n], ref['flags'][k:k + n]), 'flag words of image %d' % i
        assert np.array_equal(words[i, :n], ref['open'][k:k + n]), 'open words of image %d' % i
        assert (flags[i, n:] == INVALID).all() and (words[i, n:] == 0).all()
        k += n
    ev.enqueue()
    r = ev.result()
    _assert_matches_ref(r, ref)
    assert r['n'] == int(((ref['flags'] >> 31) == 0).sum()) and r['nan_scores'] == int(np.isnan(ref['scores']).sum()) > 0
    cls, sc, fl, op = ev.sorted()
    order = O.sorted_order(ref['scores'], ref['classes'], ref['flags'], C + 1)
    assert np.array_equal(fl, ref['flags'][order]) and np.array_equal(op, ref['open'][order]) and np.array_equal(cls, ref['classes'][order])
    if n_unknown and M > 1:
        o = ref['open'][(ref['flags'] >> 31) == 0]
        assert (o == 7).any() and (o == 3).any() and (o == 1).any() and (o == 0).any()       # IoU 1, exactly 0.5, exactly 0.25, below
        assert ref['a_ose'][0] > ref['a_ose'][2] > 0 and (ref['open_at'] < ref['open_total']).any()
    m = ev.evaluate()
    assert m['OpenSet/A-OSE@0.5IOU'] == ref['a_ose'][1] and np.array_equal(m['OpenSet/WI@0.5IOU'], ref['wi'][1], equal_nan=True)
    assert np.array_equal(m['OpenSet/U-Recall@0.25IOU'], ref['u_recall'][0], equal_nan=True)
    assert np.array_equal(m['Recall@0.9IOU/c2'], ref['recall'][2, 2], equal_nan=True) and 'AP@0.5IOU/c4' in m and 'AP@0.5IOU/c5' not in m
    known = ref['ap'][1, :C]
    assert np.array_equal(m['Precision/mAP@0.5IOU'], np.nanmean(known) if np.isfinite(known).any() else np.nan, equal_nan=True)


def test_no_ground_truth_columns_and_no_detections():
    """M = 0 (an empty ground-truth tensor) and count = 0 everywhere: every count is 0, WI is NaN"""
    C = 3
    ev = _open(C, (0.5, 0.75), capacity=64)
    det = torch.zeros(2, 5, 6, device=DEV)
    det[:, :, 2:4], det[:, :, 4], det[:, :, 5] = 10.0, 0.5, 1.0
    flags, words = ev.add_batch(det, torch.tensor([5, 3], dtype=torch.int32), torch.zeros(2, 0, 4), torch.zeros(2, 0, dtype=torch.int64))
    assert _u32(flags).reshape(-1).tolist() == [0] * 8 + [INVALID] * 2 and not words.any()
    ev.add_batch(det, torch.zeros(2, dtype=torch.int32), torch.zeros(2, 0, 4), torch.zeros(2, 0, dtype=torch.int64))
    ev.enqueue()
    r = ev.result()
    assert r['n'] == 8 and r['n_det'].tolist() == [[8, 0, 0, 0]] * 2 and not r['tp'].any() and (r['pos'] == -1).all()
    assert np.isnan(r['wi']).all() and np.isnan(r['u_recall']).all() and r['a_ose'].tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------ sorted counts
def _tile():
    from ood_object_detection_amd import _lib
    return _lib.load().effdet_eval_scale_sort_tile()


def _load(ev, scores, classes, flags, words, gt_count):
    """put accumulated entries into the evaluator's device buffers directly (what add_batch calls would have left there)"""
    n = len(scores)
    ev.clear()
    ev._bufs[0][:n] = torch.from_numpy(np.asarray(scores, np.float32)).to(DEV)
    ev._bufs[1][:n] = torch.from_numpy(np.asarray(classes, np.int32)).to(DEV)
    ev._bufs[2][:n] = torch.from_numpy(np.asarray(flags, np.int64).astype(np.uint32).view(np.int32)).to(DEV)
    ev._open[:n] = torch.from_numpy(np.asarray(words, np.int64).astype(np.uint32).view(np.int32)).to(DEV)
    ev._state[0] = n
    ev._gt_count.copy_(torch.from_numpy(np.asarray(gt_count, np.int32)))
    ev._gt_imgs.copy_(torch.from_numpy((np.asarray(gt_count) > 0).astype(np.int32)))


def _segments(n, seg, tile, seed):
    """n entries over 8 classes (7 = the unknown one) in random arrival order, 64 distinct scores (ties everywhere), random open
    words.  Class 1 keeps exactly `seg` entries in the sorted list (none of its entries is dropped); with n > 2 tiles class 0 has
    tile - 1000 entries before the drop, so class 1 straddles a sort tile in the sorted order.  Its second and third true positives
    are alone at the two lowest scores: positions seg - 2 and seg - 1, the two sides of the 2048-entry chunk edge.
      class 0  n_gt 8: 0.625 n_gt is an integer           class 4  n_gt 4, its top entry a true positive alone at the top score
      class 1  n_gt 4, 3 true positives: the exact tie     class 5  n_gt 4, its top entry ignored, alone at the top score
      class 2  n_gt 100, 7 true positives: clipped by tp   class 6  ground truth, no entry
      class 3  no true positive                            class 7  entries, no ground truth"""
    rs = np.random.RandomState(seed)
    n0 = tile - 1000 if n > 2 * tile else max(n - seg - 300, 10)
    rest = n - n0 - seg
    assert rest >= 50
    classes = np.concatenate([np.zeros(n0, int), np.ones(seg, int), rs.choice([2, 3, 4, 5, 7, -1, 8], rest)])
    classes[n0 + seg:n0 + seg + 12] = [2, 3, 4, 5, 7, 2, 3, 4, 5, 7, -1, 8]
    scores = (rs.randint(0, 64, n) / np.float32(64)).astype(np.float32)
    u = rs.uniform(size=n)
    flags = np.where(u < 0.1, 1 << 16, np.where(u < 0.13, 1 << 31, 0)).astype(np.int64)
    flags[(classes == 1) & (flags == 1 << 31)] = 0
    for c, k in ((0, 9), (1, 1), (2, 7), (4, 5), (5, 4), (7, 6)):
        idx = np.nonzero((classes == c) & (flags == 0))[0]
        flags[rs.permutation(idx)[:k]] = 1
    scores[n0 + seg - 2], scores[n0 + seg - 1] = -1.0, -2.0
    flags[n0 + seg - 2:n0 + seg] = 1
    for c, word in ((4, 1), (5, 1 << 16)):
        i = np.nonzero(classes == c)[0][1]
        scores[i], flags[i] = 2.0, word
    words = rs.randint(0, 2, n)
    perm = rs.permutation(n)
    return scores[perm], classes[perm], flags[perm], words[perm], np.array([8, 4, 100, 6, 4, 4, 5, 0])


@pytest.mark.parametrize('which,seg', [('tile-1', 2047), ('tile', 2048), ('tile+1', 2049), ('3*tile+17', 2047), ('3*tile+17', 2048),
                                       ('3*tile+17', 2049)])
def test_sorted_counts_around_the_tiles(which, seg):
    tile = _tile()
    n = eval(which, {'tile': tile})
    scores, classes, flags, words, gt_count = _segments(n, seg, tile, n + seg)
    ev = _open(7, capacity=max(n, 2 * tile + 5))
    _load(ev, scores, classes, flags, words, gt_count)
    order = O.sorted_order(scores, classes, flags, 8)
    at = np.nonzero(classes[order] == 1)[0]
    assert len(at) == seg
    if n > 2 * tile:
        assert at[0] < tile <= at[-1]
    seen = {}
    for level in (0.625, 0.1, 1.0):
        ev.enqueue(recall_level=level)
        r = ev.result()
        ref = O.counts_from_entries(scores, classes, flags, words, gt_count, 8, 1, level)
        for k in O.MATRICES:
            assert np.array_equal(r[k], ref[k]), (level, k, r[k], ref[k])
        ap = R.ap_from_entries(scores, classes, flags, gt_count, 8, 1)
        assert np.array_equal(np.isnan(r['ap']), np.isnan(ap)) and np.allclose(r['ap'], ap, rtol=0, atol=1e-12, equal_nan=True)
        seen[level] = ref
        cls, sc, fl, op = ev.sorted()
        assert np.array_equal(fl, (flags.astype(np.uint32))[order]) and np.array_equal(op, words.astype(np.uint32)[order])
    a, b = seen[0.625], seen[0.1]
    assert a['k_star'][0, 0] == 5 and a['k_star'][0, 1] == 2 and a['k_star'][0, 2] == 7 == a['tp'][0, 2]
    assert a['tp'][0, 3] == 0 and a['k_star'][0, 3] == 0 and a['pos'][0, 3] == 0
    assert b['k_star'][0, 4] == 1 and b['pos'][0, 4] == 0 and b['rank_at'][0, 4] == 1            # k_min = 1: 0 is not reachable
    assert b['k_star'][0, 5] == 0 and b['pos'][0, 5] == 0 and b['rank_at'][0, 5] == 0            # position 0 is ignored
    assert a['pos'][0, 6] == -1 and a['n_det'][0, 6] == 0 and a['pos'][0, 7] == -1 and a['n_det'][0, 7] > 0 and a['tp'][0, 7] == 6
    assert seen[1.0]['k_star'][0, 0] == 8 and seen[1.0]['k_star'][0, 1] == 3
    # the chunk edge: seg = 2048 puts the third true positive on the last entry of chunk 0, seg = 2049 the second there and the
    # third alone in chunk 1
    assert a['pos'][0, 1] == seg - 2 and seen[1.0]['pos'][0, 1] == seg - 1 and a['tp'][0, 1] == 3
    assert seen[1.0]['rank_at'][0, 1] == a['n_det'][0, 1] and seen[1.0]['open_at'][0, 1] == a['open_total'][0, 1]


def test_sorted_counts_of_one_class_with_70000_entries():
    """more than 256 x 256 entries in one segment; the position lies beyond entry 65 536"""
    n, rs = 70000, np.random.RandomState(9)
    scores = (rs.randint(0, 4096, n) / np.float32(4096)).astype(np.float32)
    u = rs.uniform(size=n)
    flags = np.where(u < 0.35, 1, np.where(u < 0.45, 1 << 16, 0)).astype(np.int64)
    words = rs.randint(0, 2, n)
    gt_count = np.array([30000, 0])
    ev = _open(1, capacity=n)
    _load(ev, scores, np.zeros(n, int), flags, words, gt_count)
    ev.enqueue(recall_level=0.8)
    r = ev.result()
    ref = O.counts_from_entries(scores, np.zeros(n, int), flags, words, gt_count, 2, 1, 0.8)
    for k in O.MATRICES:
        assert np.array_equal(r[k], ref[k]), (k, r[k], ref[k])
    assert ref['k_star'][0, 0] == 24000 and ref['pos'][0, 0] > 65536 and r['wi'][0] == ref['open_at'][0, 0] / ref['rank_at'][0, 0]


def test_sorted_counts_with_300_classes():
    """more than 255 classes: the class takes two digits of the key, so the sort runs a sixth pass, here with both payload words;
    tile + 1 entries, so the last one is alone in a second tile.  Classes -1 and 300 and flag bit 31 are invalid entries."""
    C1, rs = 300, np.random.RandomState(21)
    n = _tile() + 1
    scores = (rs.randint(0, 64, n) / np.float32(64)).astype(np.float32)
    classes = rs.randint(-1, C1 + 1, n)
    u = rs.uniform(size=n)
    flags = np.where(u < 0.3, 1, np.where(u < 0.4, 1 << 16, np.where(u < 0.45, 1 << 31, 0))).astype(np.int64)
    words = rs.randint(0, 2, n)
    gt_count = np.array([int(((flags == 1) & (classes == c)).sum()) + rs.randint(0, 3) for c in range(C1)])
    gt_count[C1 - 1] = 0
    ev = _open(C1 - 1, capacity=n + 7)
    _load(ev, scores, classes, flags, words, gt_count)
    ev.enqueue(recall_level=0.625)
    r = ev.result()
    ref = O.counts_from_entries(scores, classes, flags, words, gt_count, C1, 1, 0.625)
    for k in O.MATRICES:
        assert np.array_equal(r[k], ref[k]), (k, np.nonzero(r[k] != ref[k]))
    assert len(O.MATRICES) == 7 and (ref['n_det'][0, 256:] > 0).any() and (ref['tp'][0, 256:] > 0).any() and (ref['open_total'][0] > 0).any()
    order = O.sorted_order(scores, classes, flags, C1)
    cls, sc, fl, op = ev.sorted()
    assert np.array_equal(fl, (flags.astype(np.uint32))[order]) and np.array_equal(op, words.astype(np.uint32)[order])


def test_sixteen_thresholds_an_entry_ignored_everywhere_is_dropped_from_the_open_counts():
    thresholds = [round(0.2 + 0.05 * i, 2) for i in range(16)]
    gt = np.array([[0, 0, 10, 10], [0, 0, 10, 10], [50, 50, 60, 60], [50, 50, 60, 60]], np.float32)
    det = np.array([[0, 0, 10, 10], [50, 50, 60, 60], [50, 50, 60, 70]], np.float32)
    im = dict(gt_boxes=gt, gt_classes=np.array([0, 1, 0, 1]), gt_difficult=np.array([True, False, False, False]), det_boxes=det,
              det_scores=np.array([0.9, 0.8, 0.7], np.float32), det_classes=np.array([0, 0, 0]))
    ref = O.evaluate([im], 1, thresholds, 0.8)
    assert ref['flags'].tolist() == [0xFFFF0000, 0xFFFF, 0] and ref['open'].tolist() == [0, 0xFFFF, 0x7F]
    ev = _open(1, thresholds, capacity=16)
    flags, words = ev.add_batch(*_dev(O.pack([im], 4, 4)))
    assert _u32(flags)[0].tolist() == [0xFFFF0000, 0xFFFF, 0, INVALID] and _u32(words)[0].tolist() == [0, 0xFFFF, 0x7F, 0]
    ev.enqueue()
    r = ev.result()
    _assert_matches_ref(r, ref)
    assert r['n'] == 2 and r['open_total'][:, 0].tolist() == [2] * 7 + [1] * 9 and r['n_det'][:, 0].tolist() == [2] * 16


# ------------------------------------------------------------------------------------------------ mechanics
def _mech_case():
    C, M = 5, 64
    return O.open_case(77, 6, 40, C, M, 20), C, M, O.CASE_THRESHOLDS


def _run_split(ev, images, parts, M):
    ev.clear()
    for idx in np.array_split(np.arange(len(images)), parts):
        ev.add_batch(*_dev(O.pack([images[i] for i in idx], 40, M)))
    ev.enqueue()
    return ev.result()['block']


def test_result_block_is_bit_identical_across_runs_and_splits():
    images, C, M, thresholds = _mech_case()
    ev = _open(C, thresholds, capacity=512)
    blocks = [_run_split(ev, images, parts, M) for parts in (1, 2, len(images), 1)]
    for b in blocks[1:]:
        assert np.array_equal(b, blocks[0])
    assert np.array_equal(_run_split(_open(C, thresholds, capacity=1 << 14), images, 2, M), blocks[0])
    assert blocks[0][0] == int(((O.evaluate(images, C, thresholds)['flags'] >> 31) == 0).sum())


def test_add_batch_and_enqueue_in_a_captured_graph():
    images, C, M, thresholds = _mech_case()
    ev = _open(C, thresholds, capacity=512)
    first, second = _dev(O.pack(images[:4], 40, M)), _dev(O.pack(images[4:], 40, M))
    ev.add_batch(*first)
    ev.add_batch(*second)
    ev.enqueue()
    eager = ev.result()['block']
    ev.clear()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ev.add_batch(*first)
        ev.add_batch(*second)
        ev.enqueue()
    for _ in range(2):
        ev.clear()
        ev._result.zero_()
        graph.replay()
        assert np.array_equal(ev.result()['block'], eager)


def test_overflow_is_reported_and_clear_allows_reuse():
    images, C, M, thresholds = _mech_case()
    total = int(((O.evaluate(images, C, thresholds)['flags'] >> 31) == 0).sum())
    ev = _open(C, thresholds, capacity=total - 7)
    ev.add_batch(*_dev(O.pack(images[:3], 40, M)))
    ev.add_batch(*_dev(O.pack(images[3:], 40, M)))
    ev.enqueue()
    with pytest.raises(RuntimeError, match=r'\b7\b.*\b%d\b' % (total - 7)):
        ev.result()
    ev.clear()
    ev.add_batch(*_dev(O.pack(images[:3], 40, M)))
    ev.enqueue()
    r = ev.result()
    _assert_matches_ref(r, O.evaluate(images[:3], C, thresholds))
    assert r['lost'] == 0


# ------------------------------------------------------------------------------------------------ relabelling
def _relabel_case():
    rs = np.random.RandomState(3)
    B, max_det, C = 5, 300, 4
    det = rs.uniform(0, 1, (B, max_det, 6)).astype(np.float32)
    det[:, :, 5] = rs.randint(-1, C + 3, (B, max_det))
    det[0, 3, 5], det[0, 7, 5], det[0, 9, 5], det[0, 11, 5] = 1, 2, 3, 4
    full = rs.normal(0, 1, (B, max_det, 2)).astype(np.float32)                # a `last_ood`-style strided view: [..., 0]
    score = full[:, :, 0]
    score[0, 3], score[0, 9], score[0, 11] = np.nan, np.inf, -np.inf
    tau = np.float32(score[0, 7])                                             # tau equals a score: >= keeps it known
    count = np.array([max_det, 0, 11, 299, 1], np.int32)
    want = det.copy()
    hit = (np.arange(max_det)[None] < count[:, None]) & (det[:, :, 5] >= 1) & (det[:, :, 5] <= C) & ~(score >= tau)
    want[:, :, 5][hit] = C + 1
    assert hit[0, 3] and not hit[0, 7] and not hit[0, 9] and hit[0, 11] and not hit[1].any() and not hit[2, 11:].any()
    return det, count, full, tau, C, want


def test_relabel_unknown_is_exact_with_host_and_device_thresholds_and_in_place():
    from ood_object_detection_amd import ood
    det, count, full, tau, C, want = _relabel_case()
    d, c, f = _dev((det, count, full))
    view = f[:, :, 0]
    assert not view.is_contiguous()
    host = ood.relabel_unknown(d, c, view, float(tau), C)
    device = ood.relabel_unknown(d, c, view, torch.tensor(tau, device=DEV), C)
    assert torch.equal(d.cpu(), torch.from_numpy(det))                                          # the input is untouched
    assert np.array_equal(host.cpu().numpy().view(np.uint32), want.view(np.uint32)) and torch.equal(host, device)
    assert torch.equal(ood.relabel_unknown(d, c.to(torch.int64), view.contiguous(), float(tau), C), host)
    out = ood.relabel_unknown(d, c, view, float(tau), C, out=d)
    assert out is d and torch.equal(d, host)


# ------------------------------------------------------------------------------------------------ end to end
def test_end_to_end_chain_threshold_relabel_open_set_evaluation():
    """tf_efficientdet_d0 at 128 px, 4 images: OODEvaluator.enqueue -> threshold_tensor() -> relabel_unknown on -energy ->
    OpenSetDetectionEvaluator, nothing read by the host in between; equal to the restatement fed the same detections and the
    threshold read back afterwards"""
    from _models import seeded_model
    from _seeded import seeded_array
    from ood_object_detection_amd import ood
    from ood_object_detection_amd.effdet.bench import DetBenchPredict
    C = 3
    model, cfg, _, _ = seeded_model('tf_efficientdet_d0', 128, C, seed=21, cls_bias=-2.0)
    x = torch.from_numpy(seeded_array(22, 'input', (4, 3, 128, 128))).to(DEV)
    bench = DetBenchPredict(model.to(DEV).float(), streams=1).to(DEV)
    det = bench(x).clone()
    count, energy = bench.last_count.clone(), bench.last_ood['energy'].clone()
    B, max_det, _ = det.shape
    assert int(count.sum()) > 8 and energy.shape == (B, max_det)
    # ground truth from the detections themselves: every fourth valid row is an object, of its own class or (every eighth) unknown
    d = det.cpu().numpy()
    cnt = count.cpu().numpy()
    M = 16
    gtb, gtc = np.zeros((B, M, 4), np.float32), np.full((B, M), -1, np.int64)
    for b in range(B):
        rows = np.arange(0, cnt[b], 4)[:M]
        gtb[b, :len(rows)] = d[b, rows][:, [1, 0, 3, 2]]
        gtc[b, :len(rows)] = np.where(np.arange(len(rows)) % 2 == 1, C + 1, d[b, rows, 5].astype(np.int64))
    oe = ood.OODEvaluator(B * max_det, B * max_det, device=DEV)
    oe.add_detections(energy[:2], count[:2], ood=False, negate=True)
    oe.add_detections(energy[2:], count[2:], ood=True, negate=True)
    oe.enqueue(0.5)
    tau = oe.threshold_tensor()
    assert tau.dim() == 0 and tau.dtype == torch.float32 and tau.device.type == 'cuda'
    relabelled = ood.relabel_unknown(det, count, -energy, tau, C)
    ev = _open(C, (0.5, 0.75), capacity=B * max_det)
    flags, words = ev.add_batch(relabelled, count, torch.from_numpy(gtb), torch.from_numpy(gtc))
    ev.enqueue()
    r = ev.result()                                                           # the first host read of the chain
    tau_host = oe.result()['threshold']
    assert float(tau) == tau_host
    want = d.copy()
    s = -energy.cpu().numpy()
    hit = (np.arange(max_det)[None] < cnt[:, None]) & (d[:, :, 5] >= 1) & (d[:, :, 5] <= C) & ~(s >= np.float32(tau_host))
    want[:, :, 5][hit] = C + 1
    assert np.array_equal(relabelled.cpu().numpy(), want) and hit.any() and not hit[np.arange(max_det)[None] < cnt[:, None]].all()
    images = []
    for b in range(B):
        m = int((gtc[b] > 0).sum())
        images.append(dict(gt_boxes=gtb[b, :m], gt_classes=gtc[b, :m] - 1, det_boxes=want[b, :cnt[b]][:, [1, 0, 3, 2]],
                           det_scores=want[b, :cnt[b], 4], det_classes=want[b, :cnt[b], 5].astype(np.int64) - 1))
    ref = O.evaluate(images, C, (0.5, 0.75), 0.8)
    _assert_matches_ref(r, ref)
    k = 0
    for b in range(B):
        assert np.array_equal(_u32(flags)[b, :cnt[b]], ref['flags'][k:k + cnt[b]]) and np.array_equal(_u32(words)[b, :cnt[b]], ref['open'][k:k + cnt[b]])
        k += cnt[b]
    assert r['tp'].sum() > 0
