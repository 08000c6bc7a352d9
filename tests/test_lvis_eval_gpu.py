"""csrc/lvis_eval.hip on the device (-m gpu): the image rank with ties, the cap over all categories, the federated filter, the
bitsets at the word edges of C, matching in rank order and the not-exhaustive rule, then the append, the sort and AP / AR of the
COCO unit on top, against tests/_lvis_eval_ref.py and against themselves (bit-identical runs).

Flag words, ranks, npig, the kept count and the sorted order are compared EXACTLY: both sides compute the IoU by the same float32
operations.  precision, AP and AR are compared BITWISE with the restatement's sequential sum (every term is one float64 division,
AP is R additions in ascending r on both sides).  Every randomized case is checked to contain rank-cut, filter-dropped and
nel-ignored detections, except where its construction excludes one (neg = all categories or no neg list: nothing to filter; no
nel list: nothing to ignore), which the case then asserts."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _coco_eval_ref as K
import _lvis_eval_ref as L
from test_lvis_eval_host import _im, _lvis_dict, check_abi_refusals

DEV = 'cuda:0'
F = np.float32


def _cats(C, freq=None):
    return [dict(id=i + 1, name='c%d' % i, **({'frequency': freq[i]} if freq else {})) for i in range(C)]


def _evaluator(C, freq=None, **kw):
    from ood_object_detection_amd.effdet.evaluation import LvisDetectionEvaluator
    return LvisDetectionEvaluator(_cats(C, freq), device=DEV, **kw)


def _pack(images, max_det, M, Kn=None):
    return [torch.from_numpy(a).to(DEV) if a is not None else None for a in L.pack(images, max_det, M, Kn=Kn)]


def _bits(a):
    a = np.asarray(a, np.float64)
    return np.isnan(a), np.where(np.isnan(a), 0.0, a).view(np.uint64)


def _assert_bitwise(got, ref, what):
    (gn, gb), (rn, rb) = _bits(got), _bits(ref)
    assert got.shape == ref.shape and np.array_equal(gn, rn), what
    assert np.array_equal(gb, rb), (what, np.abs(np.nan_to_num(got) - np.nan_to_num(ref)).max())


def _check(images, C, M, max_det, splits=1, Kn=None, need=('cut', 'filtered', 'nel'), **kw):
    """the evaluator on `images` against the restatement: everything, exactly"""
    ev = _evaluator(C, capacity=len(images) * max_det + 7, keep_precision=True, **kw)
    ref = L.evaluate(images, C, kw.get('iou_thresholds', L.LVIS_THRESHOLDS), kw.get('area_ranges', L.LVIS_AREAS),
                     kw.get('max_dets', L.LVIS_MAX_DETS), kw.get('recall_thresholds', L.LVIS_REC_THRS), kw.get('min_score', 0.0))
    print('cut / filtered / nel-ignored:', ref['stats'])
    for k in ('cut', 'filtered', 'nel'):
        assert (ref['stats'][k] > 0) == (k in need), (k, ref['stats'])
    flags, ranks = [], []
    for idx in np.array_split(np.arange(len(images)), splits):
        flags.append(ev.add_batch(*_pack([images[i] for i in idx], max_det, M, Kn)).cpu().numpy().view(np.uint32))
        ranks.append(ev._last_rank.cpu().numpy())
    flags, ranks = np.concatenate(flags), np.concatenate(ranks)
    for i, im in enumerate(images):
        n = len(im['det_scores'])
        assert np.array_equal(flags[i, :n], ref['flags'][i]), ('flags', i)
        assert np.array_equal(ranks[i, :n], ref['ranks'][i]), ('ranks', i)
        assert (flags[i, n:] == 0x80000000).all() and (ranks[i, n:] == -1).all()
    ev.enqueue()
    r = ev.result()
    n = len(ref['scores'])
    assert r['n'] == n and r['lost'] == 0 and r['nan_scores'] == ref['nan_scores']        # n: the sum of the kept counts
    assert np.array_equal(r['npig'], ref['npig'])
    cls, scores, words, rk, index = ev.sorted()
    order = L.sorted_entries(ref['scores'], ref['classes'], C)
    assert np.array_equal(index, order) and np.array_equal(cls, ref['classes'][order]) and np.array_equal(scores, ref['scores'][order] + F(0))
    assert np.array_equal(words, ref['words'][order]) and np.array_equal(rk, ref['rank'][order])
    _assert_bitwise(ev.precision().cpu().numpy(), ref['precision'], 'precision')
    _assert_bitwise(r['ap'], ref['ap'], 'AP')
    _assert_bitwise(r['ar'], ref['ar'], 'AR')
    return ref


# ------------------------------------------------------------------------------------------------ matching
def _special_images():
    return [
        _im([[0, 0, 10, 10]], [0], [[50, 50, 60, 60], [0, 0, 10, 10], [70, 70, 80, 80], [20, 20, 30, 30]], [0.9, 0.8, 0.7, 0.6],
            det_cls=[2, 0, 1, 0], neg=[1], nel=[]),                                        # not judged, yet a place in the top 3
        _im([[0, 0, 10, 10]], [1], [[40, 40, 50, 50], [0, 0, 10, 10]], [0.9, 0.8], det_cls=[1, 1], neg=[], nel=[1]),      # nel: ignored / TP
        _im([[0, 0, 10, 10]], [0], [[0, 0, 10, 10]] * 3, [0.5, 0.9, 0.5], neg=[], nel=[]),             # ties; a box is taken once
        _im([[0, 0, 32, 32], [0, 0, 10, 10]], [2, 2], [[100, 100, 132, 132], [0, 0, 32, 32]], [0.9, 0.8], det_cls=[2, 2], neg=[], nel=[],
            gt_area=[1024.0, 9217.0]),                                                     # areas on the edges of the ranges
        _im([[0, 0, 10, 40], [100, 0, 110, 40]], [2, 2], [[100, 0, 110, 20], [0, 0, 10, 30]], [0.8, 0.9], det_cls=[2, 2], neg=[], nel=[]),
        _im(np.zeros((0, 4)), [], [[0, 0, 10, 10], [0, 0, 20, 20]], [0.5, 0.25], det_cls=[0, 2], neg=[2], nel=[2]),       # no boxes
        _im([[0, 0, 10, 10], [0, 0, 50, 50]], [0, 1], np.zeros((0, 4)), [], neg=[], nel=[]),                           # no detections
        _im([[0, 0, 10, 10]], [0], [[0, 0, 10, 10]] * 4, [0.9, np.nan, 0.5, 0.2], det_cls=[0, 0, 7, 0], neg=[0, 1, 2], nel=[]),
    ]


@pytest.mark.parametrize('params', [dict(), dict(iou_thresholds=[0.5], area_ranges=[L.LVIS_AREAS[0]]),
                                    dict(iou_thresholds=np.linspace(0.25, 0.95, 15))], ids=['T10_A4', 'T1_A1', 'T15'])
def test_special_cases(params):
    ref = _check(_special_images(), 3, 2, 5, splits=2, max_dets=(3,), **params)
    f, rk = ref['flags'], ref['ranks']
    assert rk[0].tolist() == [-1, 1, 2, -1] and [int(w) & 1 for w in f[0][:, 0]] == [0, 1, 0, 0] and f[0][2, 0] == 0
    assert (f[1][0, 0] >> 16) != 0 and (f[1][0, 0] & 0xFFFF) == 0 and (f[1][1, 0] & 1) == 1
    assert rk[2].tolist() == [1, 0, 2] and [int(w) & 1 for w in f[2][:, 0]] == [0, 1, 0]
    if len(params.get('iou_thresholds', L.LVIS_THRESHOLDS)) == 10:
        assert f[4][:, 0].tolist() == [0b1, 0b111111] and ref['npig'][2].tolist() == [4, 3, 1, 1]      # 1024 lies in two ranges


@pytest.mark.parametrize('M,max_det,n_det,cap', [(1, 100, 40, 25), (255, 100, 100, 60), (257, 100, 60, 40), (300, 300, 300, 200)])
def test_matching_sizes(M, max_det, n_det, cap):
    """M on both sides of the 256-thread staging loop; 300 detections in 300 slots"""
    C = 5
    images = L.random_images(100 + M, 2, C, M, n_det, n_neg=1, scores_levels=32 if M == 257 else 0, gt_classes=3)
    images[0]['gt_area'] = (L._area(images[0]['gt_boxes']) * F(0.75)).astype(F)          # segmentation area, not the box area
    assert max(len(im['det_scores']) for im in images) == n_det
    ref = _check(images, C, M, max_det, max_dets=(cap,))
    words = np.concatenate(ref['flags'])
    assert (words & 0x3FF).any() and ((words >> 16) & 0x3FF).any() and (words >> 31).any()


def test_slots_beyond_the_cap_of_300():
    """max_det 1024 with 700 rows below the count: LVIS's cut at 300 acts; the ranks of the kept rows stay below 300"""
    C, M = 8, 24
    images = L.random_images(7, 2, C, M, 700, n_neg=2, n_nel=2, gt_classes=4)
    assert max(len(im['det_scores']) for im in images) == 700
    ref = _check(images, C, M, 1024)
    assert ref['stats']['cut'] > 300 and 250 < max(r.max() for r in ref['ranks']) <= 299


@pytest.mark.parametrize('C,n_neg,Kn,need', [(3, 1, None, ('cut', 'filtered', 'nel')), (32, 0, 0, ('cut', 'filtered', 'nel')),
                                             (33, 33, None, ('cut', 'nel')), (65, 2, None, ('cut', 'filtered', 'nel')),
                                             (1203, 6, 9, ('cut', 'filtered', 'nel'))], ids=['C3_Kn1', 'C32_Kn0', 'C33_KnC', 'C65', 'C1203'])
def test_category_sets_at_the_bitset_word_edges(C, n_neg, Kn, need):
    """C = 32 / 33 / 65: the last class is bit 31 of a word / bit 0 of the next; Kn = 0 (the empty set: only pos is judged), 1, C"""
    images = L.random_images(200 + C, 3, C, 12, 40, n_neg=n_neg, n_nel=2, gt_classes=3, scores_levels=64 if C == 65 else 0)
    for im in images[:2]:                                                     # the word edges: the last class has a box, a detection, and is nel
        im['gt_classes'][:1] = C - 1
        im['det_classes'][:2] = C - 1
        im['nel'] = sorted(set(im['nel']) | {C - 1})
    ref = _check(images, C, 12, 40, Kn=Kn, need=need, max_dets=(25,))
    assert ref['npig'][C - 1, 0] > 0 and any((r[:2] >= 0).any() for r in ref['ranks'])


def test_null_lists_judge_every_category_and_ignore_none():
    images = L.random_images(11, 3, 6, 12, 40, n_neg=None, n_nel=None)
    _check(images, 6, 12, 40, need=('cut',), max_dets=(25,))
    for im in images:                                                         # a nel list alone
        im['nel'] = [0, 3]
    _check(images, 6, 12, 40, need=('cut', 'nel'), max_dets=(25,))


def test_a_row_permutation_gives_the_same_word_per_detection():
    C, M, max_det = 6, 12, 40
    images = L.random_images(13, 3, C, M, max_det, n_neg=2)
    assert all(len(set(im['det_scores'].tolist())) == len(im['det_scores']) for im in images)          # distinct scores
    ev = _evaluator(C, capacity=1024, max_dets=(25,))
    det, cnt, *rest = _pack(images, max_det, M)
    f0 = ev.add_batch(det, cnt, *rest).cpu().numpy()
    r0 = ev._last_rank.cpu().numpy()
    ev.enqueue()
    block = ev.result()['block']
    ev.clear()
    perm = torch.stack([torch.randperm(max_det, generator=torch.Generator().manual_seed(b)) for b in range(len(images))]).to(DEV)
    full = torch.full_like(cnt, max_det)                                      # the rows of zeros behind the count are not valid either way
    f1 = ev.add_batch(torch.gather(det, 1, perm[:, :, None].expand(-1, -1, 6)), full, *rest).cpu().numpy()
    r1 = ev._last_rank.cpu().numpy()
    p = perm.cpu().numpy()
    for b in range(len(images)):
        assert np.array_equal(f1[b], f0[b][p[b]]) and np.array_equal(r1[b], r0[b][p[b]])
    ev.enqueue()
    got = ev.result()['block']
    assert np.array_equal(got[8:], block[8:]) and got[0] == block[0] > 0                               # AP, AR and npig: the same bits


def test_equals_the_coco_evaluator_where_the_protocols_coincide():
    """neg = all categories, no nel, no crowd, descending rows, at most 300 detections an image: the flag words and the result
    block of `CocoDetectionEvaluator(max_dets=(300,))` on the same tensors, bit for bit"""
    from ood_object_detection_amd.effdet.evaluation import CocoDetectionEvaluator
    C, M, max_det = 5, 20, 120
    images = K.random_images(17, 5, C, M, max_det, crowd_frac=0.0, scores_levels=32)
    det, cnt, gtb, gtc, _, _ = [torch.from_numpy(a).to(DEV) if a is not None else None for a in K.pack(images, max_det, M)]
    neg = torch.arange(1, C + 1, device=DEV).repeat(len(images), 1)
    lv = _evaluator(C, capacity=1024)
    co = CocoDetectionEvaluator(_cats(C), max_dets=(300,), capacity=1024, device=DEV)
    fl, fc = lv.add_batch(det, cnt, gtb, gtc, None, neg, None), co.add_batch(det, cnt, gtb, gtc)
    assert torch.equal(fl, fc) and bool((fl >= 0).any())
    lv.enqueue()
    co.enqueue()
    a, b = lv.result(), co.result()
    assert np.array_equal(a['block'], b['block']) and a['n'] > 100 and np.nanmax(a['ap']) > 0


def test_images_in_any_split_give_the_same_bits_and_runs_repeat():
    C, M, max_det = 6, 20, 50
    images = L.random_images(9, 9, C, M, max_det, n_neg=2, scores_levels=16)
    ev = _evaluator(C, capacity=4096, keep_precision=True, max_dets=(10, 30))

    def run(e, parts):
        e.clear()
        for idx in np.array_split(np.arange(len(images)), parts):
            e.add_batch(*_pack([images[i] for i in idx], max_det, M))
        e.enqueue()
        return e.result()['block'], e.precision().cpu().numpy().copy()
    blocks = [run(ev, parts) for parts in (1, 3, 9, 1)]
    blocks.append(run(_evaluator(C, capacity=1 << 16, keep_precision=True, max_dets=(10, 30)), 2))
    for b, p in blocks[1:]:
        assert np.array_equal(b, blocks[0][0]) and np.array_equal(_bits(p)[1], _bits(blocks[0][1])[1])
    ref = L.evaluate(images, C, max_dets=(10, 30))
    assert all(ref['stats'][k] > 0 for k in ('cut', 'filtered', 'nel')), ref['stats']
    _assert_bitwise(blocks[0][0][8:8 + ref['ap'].size].view(np.float64).reshape(ref['ap'].shape), ref['ap'], 'AP')


# ------------------------------------------------------------------------------------------------ mechanics
def test_add_batch_and_enqueue_in_a_captured_graph():
    C, M, max_det = 6, 20, 50
    images = L.random_images(21, 6, C, M, max_det, n_neg=2)
    ev = _evaluator(C, capacity=4096, max_dets=(30,))
    first, second = _pack(images[:4], max_det, M), _pack(images[4:], max_det, M)
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
    assert eager[0] > 50


def test_overflow_is_reported_and_clear_allows_reuse():
    C, M, max_det = 3, 8, 100
    images = L.random_images(31, 12, C, M, max_det, n_neg=3, n_nel=1)
    total = sum(int((L.prepare(im, C, 300)[0] >= 0).sum()) for im in images)
    ev = _evaluator(C, capacity=total - 200)
    ev.add_batch(*_pack(images[:7], max_det, M))
    ev.add_batch(*_pack(images[7:], max_det, M))
    ev.enqueue()
    with pytest.raises(RuntimeError, match=r'\b200\b.*\b%d\b' % (total - 200)):
        ev.result()
    ev.clear()
    ev.add_batch(*_pack(images[:5], max_det, M))
    ev.enqueue()
    r = ev.result()
    ref = L.evaluate(images[:5], C)
    assert r['n'] == len(ref['scores']) and r['lost'] == 0
    _assert_bitwise(r['ap'], ref['ap'], 'AP')


def test_abi_refusals_with_the_device_present():
    from ood_object_detection_amd import _lib
    check_abi_refusals(_lib.load())
    ev = _evaluator(2, capacity=16)
    z = torch.zeros
    with pytest.raises(ValueError):
        ev.add_batch(z(2, 4, 5), z(2), z(2, 1, 4), z(2, 1))
    with pytest.raises(ValueError):
        ev.add_batch(z(2, 4, 6), z(2), z(2, 1, 4), z(2, 1), neg_cls=z(3, 2))
    with pytest.raises(ValueError):
        ev.add_batch(z(2, 4, 6), z(2), z(2, 1, 4), z(2, 1), gt_area=z(2, 2))
    with pytest.raises(RuntimeError):
        ev.add_batch(z(1, 4, 6), z(1), z(1, 1700, 4), z(1, 1700))             # 40 M beyond 64 KiB of LDS: -22
    with pytest.raises(RuntimeError):
        ev.add_batch(z(1, 2049, 6), z(1), z(1, 1, 4), z(1, 1))                # max_det beyond 2048: -22
    with pytest.raises(RuntimeError):
        ev.precision()
    ev.add_batch(z(1, 2048, 6), z(1), z(1, 1, 4), z(1, 1))                    # the limit itself runs
    ev.enqueue()
    assert ev.result()['n'] == 0


# ------------------------------------------------------------------------------------------------ the evaluators on top
def test_evaluate_names_the_thirteen_lvis_figures():
    C = 6
    freq = ['r', 'c', 'f', 'c', 'f', 'f']
    images = L.random_images(51, 8, C, 20, 40, n_neg=2)
    ev = _evaluator(C, freq, capacity=1024, max_dets=(30,))
    ev.add_batch(*_pack(images, 40, 20))
    out = ev.evaluate()
    ref = L.evaluate(images, C, max_dets=(30,))
    want = L.summarize(ref['ap'], ref['ar'], freq)
    names = ['AP', 'AP50', 'AP75', 'APs', 'APm', 'APl', 'APr', 'APc', 'APf', 'AR@30', 'ARs@30', 'ARm@30', 'ARl@30']
    assert np.array_equal(out['stats'], want) and [out[k] for k in names] == want.tolist() and want[0] > 0 and (want[6:9] >= 0).all()
    per_class = np.array([out['AP/c%d' % c] for c in range(C)])
    assert np.allclose(np.nanmean(per_class), want[0], rtol=0, atol=1e-12)
    plain = _evaluator(C, capacity=1024, max_dets=(30,))                      # categories without `frequency`: the group figures are -1
    plain.add_batch(*_pack(images, 40, 20))
    assert plain.evaluate()['stats'][6:9].tolist() == [-1, -1, -1]


def test_lvis_evaluator_end_to_end_on_a_synthetic_dict():
    from ood_object_detection_amd.effdet.evaluator import LvisEvaluator
    C, M, max_det = 5, 12, 30
    freq = ['r', 'c', 'f', 'f', 'c']
    images = L.random_images(61, 7, C, M, max_det, n_neg=2)
    anns = []
    for i, im in enumerate(images):
        im['gt_area'] = L._area(im['gt_boxes']) * F(0.5)
        anns += [dict(image_id=100 + i, bbox=[float(b[1]), float(b[0]), float(b[3] - b[1]), float(b[2] - b[0])], category_id=int(c) + 1,
                      area=float(a)) for b, c, a in zip(im['gt_boxes'], im['gt_classes'], im['gt_area'])]
    data = dict(images=[dict(id=100 + i, neg_category_ids=[c + 1 for c in im['neg']], not_exhaustive_category_ids=[c + 1 for c in im['nel']])
                        for i, im in enumerate(images)],
                annotations=anns, categories=[dict(id=c + 1, name='c%d' % c, frequency=freq[c]) for c in range(C)])
    det = torch.from_numpy(L.pack(images, max_det + 3, M)[0])                 # rows of zeros behind the detections
    order = ([4, 0, 6], [1, 5], [3, 2])
    ev = LvisEvaluator(data, device=DEV)
    for idx in order:                                                         # any order of the images
        ev.add_predictions(det[idx].to(DEV), dict(img_idx=torch.tensor(idx, device=DEV)))
    metric = ev.evaluate()
    ref = L.evaluate([images[i] for idx in order for i in idx], C)
    want = L.summarize(ref['ap'], ref['ar'], freq)
    assert metric == want[0] and np.array_equal(ev.metrics['stats'], want) and metric > 0
    assert all(ref['stats'][k] > 0 for k in ('filtered', 'nel')), ref['stats']
    assert int(ev._evaluator._state[0]) == 0                                  # evaluate() resets
    yx = LvisEvaluator(data, pred_yxyx=True, device=DEV)
    for idx in order:
        yx.add_predictions(det[idx][:, :, [1, 0, 3, 2, 4, 5]].to(DEV), dict(img_idx=torch.tensor(idx)))
    assert yx.evaluate() == metric
    small = LvisEvaluator(_lvis_dict(), device=DEV)                           # sparse category ids 2, 5, 9
    small.add_predictions(torch.tensor([[[10., 20., 40., 60., 0.9, 9.], [0., 0., 5., 5., 0.8, 5.]]], device=DEV), dict(img_idx=torch.tensor([0])))
    assert small.evaluate() == pytest.approx(1.0, abs=1e-12) and np.isnan(small.metrics['AP/two'])


def test_detbench_predict_batch_feeds_the_evaluator():
    """one tf_efficientdet_d0 batch at 128 px: detections and counts go from DetBenchPredict to add_batch as device tensors; the
    ground truth is made of the images' own top detections (on the device), the lists of their classes"""
    from _models import seeded_model
    from _seeded import seeded_array
    from ood_object_detection_amd.effdet.bench import DetBenchPredict
    model, cfg, _, _ = seeded_model('tf_efficientdet_d0', 128, 20, seed=11)
    bench = DetBenchPredict(model.to(DEV).float()).to(DEV)
    det = bench(torch.from_numpy(seeded_array(11, 'input', (2, 3, 128, 128))).to(DEV))
    count = bench.last_count
    gt_boxes = det[:, :6, [1, 0, 3, 2]].contiguous()
    gt_cls = det[:, :6, 5].to(torch.int64)
    neg_cls = det[:, 6:12, 5].to(torch.int64)                                 # checked absent: the classes of the next six detections
    nel_cls = det[:, 6:8, 5].to(torch.int64)
    ev = _evaluator(20, capacity=512, min_score=0.001, max_dets=(60,))
    flags = ev.add_batch(det, count, gt_boxes, gt_cls, None, neg_cls, nel_cls)
    ev.enqueue()
    r = ev.result()                                                           # the first host read
    d, n = det.cpu().numpy(), count.cpu().numpy()
    images = [dict(det_boxes=d[b, :n[b]][:, [1, 0, 3, 2]], det_scores=d[b, :n[b], 4], det_classes=d[b, :n[b], 5].astype(np.int64) - 1,
                   gt_boxes=d[b, :6][:, [1, 0, 3, 2]], gt_classes=d[b, :6, 5].astype(np.int64) - 1,
                   neg=(d[b, 6:12, 5].astype(np.int64) - 1).tolist(), nel=(d[b, 6:8, 5].astype(np.int64) - 1).tolist()) for b in range(2)]
    ref = L.evaluate(images, 20, min_score=0.001, max_dets=(60,))
    print('cut / filtered / nel-ignored:', ref['stats'])
    f = flags.cpu().numpy().view(np.uint32)
    for b in range(2):
        assert np.array_equal(f[b, :n[b]], ref['flags'][b]) and (f[b, n[b]:] == 0x80000000).all()
    _assert_bitwise(r['ap'], ref['ap'], 'AP')
    _assert_bitwise(r['ar'], ref['ar'], 'AR')
    assert np.nanmax(r['ap']) > 0.5 and r['n'] == len(ref['scores']) > 0
