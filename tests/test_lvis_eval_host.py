"""The LVIS federated evaluation without a GPU: tests/_lvis_eval_ref.py pinned by worked examples with hand-computed answers, held
equal to tests/_coco_eval_ref.py where the two protocols coincide, the argument checks of csrc/lvis_eval.hip's C ABI and of the
Python class, `lvis_ground_truth`, and lvis-api's `LVISEval` where it happens to be installed."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import _coco_eval_ref as K
import _lvis_eval_ref as L

F = np.float32
ALL = [L.LVIS_AREAS[0]]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _im(gt, gt_cls, det, scores, det_cls=None, neg=None, nel=None, **kw):
    det = np.asarray(det, F).reshape(-1, 4)
    return dict(gt_boxes=np.asarray(gt, F).reshape(-1, 4), gt_classes=np.asarray(gt_cls, np.int64), det_boxes=det,
                det_scores=np.asarray(scores, F), det_classes=np.zeros(len(det), np.int64) if det_cls is None else np.asarray(det_cls),
                neg=neg, nel=nel, **kw)


def _bits(a):
    a = np.asarray(a, np.float64)
    return np.isnan(a), np.where(np.isnan(a), 0.0, a).view(np.uint64)


def _same(a, b):
    (an, ab), (bn, bb) = _bits(a), _bits(b)
    return a.shape == b.shape and np.array_equal(an, bn) and np.array_equal(ab, bb)


# ------------------------------------------------------------------------------------------------ worked examples
def test_a_category_that_is_not_judged_uses_up_a_place_in_the_top_k():
    """one box of class 0, class 1 checked absent, class 2 unknown to the image; max_dets (3,).  .9 class 2: rank 0, then dropped
    by the filter - neither true nor false positive; .8 class 0 on the box: rank 1, TP; .7 class 1: rank 2, FP; .6 class 0, a
    stray: rank 3 >= 3, cut although only two judged detections stand before it"""
    im = _im([[0, 0, 10, 10]], [0], [[50, 50, 60, 60], [0, 0, 10, 10], [70, 70, 80, 80], [20, 20, 30, 30]], [0.9, 0.8, 0.7, 0.6],
             det_cls=[2, 0, 1, 0], neg=[1])
    f, rank, npig, st = L.match_image(im, 3, [0.5], ALL, cap=3)
    assert rank.tolist() == [-1, 1, 2, -1] and f[:, 0].tolist() == [1 << 31, 1, 0, 1 << 31]
    assert npig.tolist() == [[1], [0], [0]] and st == dict(cut=1, filtered=1, nel=0)
    r = L.evaluate([im], 3, [0.5], ALL, (3,))
    assert r['scores'].tolist() == [F(0.8), F(0.7)] and r['classes'].tolist() == [0, 1] and r['rank'].tolist() == [1, 2]
    assert abs(r['ap'][0, 0, 0, 0] - 1) < 1e-15 and np.isnan(r['ap'][0, 1:]).all()       # class 1 has a false positive and no box: NaN
    # with a cap of 4 the stray is a false positive behind the true positive: precision at recall 1 is still 1
    f, rank, _, st = L.match_image(im, 3, [0.5], ALL, cap=4)
    assert rank.tolist() == [-1, 1, 2, 3] and f[:, 0].tolist() == [1 << 31, 1, 0, 0] and st['cut'] == 0
    # without a neg list every category is judged: the class-2 detection is a false positive
    im['neg'] = None
    assert L.match_image(im, 3, [0.5], ALL, cap=3)[0][:, 0].tolist() == [0, 1, 0, 1 << 31]


def test_not_exhaustive_category_unmatched_is_ignored_matched_is_a_true_positive():
    boxes = [[0, 0, 10, 10], [40, 40, 50, 50]]
    im = _im([[0, 0, 10, 10]], [0], boxes, [0.9, 0.8], nel=[0])
    f, _, _, st = L.match_image(im, 1, [0.5, 0.75], ALL)
    assert f[:, 0].tolist() == [0b11, 0b11 << 16] and st['nel'] == 1
    im['nel'] = []
    assert L.match_image(im, 1, [0.5, 0.75], ALL)[0][:, 0].tolist() == [0b11, 0]          # exhaustive: a false positive
    # AP: (TP, ignored) gives precision 1 everywhere; (TP, FP) too (the FP comes after recall 1); (FP, TP) gives 1/2
    im = _im([[0, 0, 10, 10]], [0], boxes[::-1], [0.9, 0.8], nel=[0])
    assert abs(L.evaluate([im], 1, [0.5], ALL)['ap'][0, 0, 0, 0] - 1) < 1e-15
    im['nel'] = None
    assert abs(L.evaluate([im], 1, [0.5], ALL)['ap'][0, 0, 0, 0] - 0.5) < 1e-15


def test_a_matched_box_is_never_matched_again():
    im = _im([[0, 0, 10, 10]], [0], [[0, 0, 10, 10]] * 3, [0.9, 0.8, 0.7])
    assert L.match_image(im, 1, [0.5], ALL)[0][:, 0].tolist() == [1, 0, 0]
    # an ignored box (area 100 is not `large`) is taken too: the second detection is unmatched there, and ignored by its own area
    f = L.match_image(im, 1, [0.5], L.LVIS_AREAS)[0]
    assert f[:, 3].tolist() == [1 << 16] * 3 and f[:, 1].tolist() == [1, 0, 0]


def test_shuffled_rows_give_the_same_word_per_detection():
    """distinct scores: the image rank, and with it every decision, belongs to the detection and not to its row"""
    for k, im in enumerate(L.random_images(3, 3, 4, 12, 30)):
        n = len(im['det_scores'])
        assert len(set(im['det_scores'].tolist())) == n
        f, rank, npig, _ = L.match_image(im, 4, cap=20)
        perm = np.random.RandomState(k).permutation(n)
        sh = dict(im, det_boxes=im['det_boxes'][perm], det_scores=im['det_scores'][perm], det_classes=im['det_classes'][perm])
        f2, rank2, npig2, _ = L.match_image(sh, 4, cap=20)
        assert np.array_equal(f2, f[perm]) and np.array_equal(rank2, rank[perm]) and np.array_equal(npig2, npig)
        assert (f & 0x3FF).any() and (rank < 0).any()


def test_equal_scores_the_earlier_slot_ranks_first():
    im = _im([[0, 0, 10, 10]], [0], [[0, 0, 10, 10], [0, 0, 10, 10], [0, 0, 10, 10]], [0.5, 0.9, 0.5])
    f, rank, _, _ = L.match_image(im, 1, [0.5], ALL)
    assert rank.tolist() == [1, 0, 2] and f[:, 0].tolist() == [0, 1, 0]
    im['det_scores'] = np.array([0.5, 0.5, 0.5], F)
    f, rank, _, _ = L.match_image(im, 1, [0.5], ALL, cap=2)
    assert rank.tolist() == [0, 1, -1] and f[:, 0].tolist() == [1, 0, 1 << 31]
    im['det_scores'] = np.array([-0.0, 0.0, -0.0], F)                          # -0.0 == +0.0: still the slot order
    assert L.match_image(im, 1, [0.5], ALL, min_score=-1.0)[1].tolist() == [0, 1, 2]


def test_area_exactly_on_an_edge_lies_in_both_ranges():
    im = _im([[0, 0, 32, 32], [0, 0, 10, 10]], [0, 0], [[0, 0, 32, 32]], [0.9], gt_area=[1024.0, 9217.0])
    f, _, npig, _ = L.match_image(im, 1, [0.5], L.LVIS_AREAS)
    assert npig.tolist() == [[2, 1, 1, 1]] and f[0].tolist() == [1, 1, 1, 1 << 16]
    im = _im([[0, 0, 32, 32]], [0], [[100, 100, 132, 132]], [0.9])            # an unmatched detection of area 1024
    assert L.match_image(im, 1, [0.5], L.LVIS_AREAS)[0][0].tolist() == [0, 0, 0, 1 << 16]
    im = _im([[0, 0, 96, 96]], [0], [[0, 0, 96, 96]], [0.9])                  # 9216: medium and large
    assert L.match_image(im, 1, [0.5], L.LVIS_AREAS)[2].tolist() == [[1, 0, 1, 1]]


def test_iou_exactly_on_a_threshold_matches():
    im = _im([[0, 0, 10, 40], [100, 0, 110, 40]], [0, 0], [[100, 0, 110, 20], [0, 0, 10, 30]], [0.8, 0.9])
    assert L._iou(im['det_boxes'][1], im['gt_boxes'][0]) == F(0.75)
    assert L.match_image(im, 1, L.LVIS_THRESHOLDS, ALL)[0][:, 0].tolist() == [0b1, 0b111111]


def test_equal_iou_goes_to_the_later_box():
    im = _im([[0, 0, 10, 10], [0, 10, 10, 20]], [0, 0], [[0, 0, 10, 20], [0, 0, 10, 10], [0, 10, 10, 20]], [0.9, 0.8, 0.7])
    assert L.match_image(im, 1, [0.5], ALL)[0][:, 0].tolist() == [1, 1, 0]


def test_invalid_rows_take_no_rank():
    im = _im([[0, 0, 10, 10]], [0], [[0, 0, 10, 10], [0, 0, 10, 10], [5, 5, 5, 9], [0, 0, 10, 10], [0, 0, 10, 10], [0, 0, 10, 10]],
             [0.0005, np.nan, 0.5, 0.3, 0.2, 0.9], det_cls=[0, 0, 0, 7, 0, 0])
    f, rank, _, st = L.match_image(im, 1, [0.5], ALL, cap=2, min_score=0.001)
    assert rank.tolist() == [-1, -1, -1, -1, 1, 0] and f[:, 0].tolist() == [1 << 31] * 4 + [0, 1] and st['cut'] == 0
    assert L.evaluate([im], 1, [0.5], ALL, (2,), min_score=0.001)['nan_scores'] == 1


def test_frequency_means_and_the_minus_one_and_nan_cells():
    """4 classes r, c, c, f; class 3 (f) has no box: NaN cells, left out of AP, and APf = -1"""
    ap = np.full((2, 4, 4, 1), np.nan)
    ap[:, 0, 0, 0], ap[:, 1, 0, 0], ap[:, 2, 0, 0] = [0.2, 0.1], [0.6, 0.4], [1.0, 0.8]
    ap[:, 0, 1, 0] = [0.3, 0.3]
    ar = np.where(np.isnan(ap), np.nan, 0.5)
    s = L.summarize(ap, ar, ['r', 'c', 'c', 'f'], thresholds=[0.5, 0.75])
    want = [3.1 / 6, 1.8 / 3, 1.3 / 3, 0.3, -1, -1, 0.15, 0.7, -1, 0.5, 0.5, -1, -1]
    assert np.allclose(s, want, rtol=0, atol=1e-15)
    assert L.summarize(ap, ar, None, thresholds=[0.5, 0.75])[6:9].tolist() == [-1, -1, -1]
    assert L.summarize(ap, ar, ['c', 'c', 'c', 'c'], thresholds=[0.5, 0.75])[6:9].tolist() == [-1, s[0], -1]
    # from detections: a class with detections and no box is NaN in AP, AR and precision
    im = _im([[0, 0, 10, 10]], [0], [[0, 0, 10, 10], [0, 0, 10, 10]], [0.9, 0.8], det_cls=[0, 1])
    r = L.evaluate([im], 2)
    assert np.isnan(r['ap'][:, 1]).all() and np.isnan(r['ar'][:, 1]).all() and np.isnan(r['precision'][:, :, 1]).all()
    assert (np.abs(r['ap'][:, 0, :2] - 1) < 1e-15).all() and np.isnan(r['ap'][:, 0, 2:]).all()         # area 100: all and small
    assert np.allclose(L.summarize(r['ap'], r['ar'], ['f', 'r']), [1, 1, 1, 1, -1, -1, -1, -1, 1, 1, 1, -1, -1], rtol=0, atol=1e-15)


def test_three_detections_two_boxes():
    """.9 TP, .8 FP, .7 TP of 2 boxes, fed as rows .7, .9, .8: precision 1, 1/2, 2/3 -> q = 1 for the 51 recall thresholds <= .5
    and 2/3 for the other 50"""
    im = _im([[0, 0, 10, 10], [20, 20, 30, 30]], [0, 0], [[20, 20, 30, 30], [0, 0, 10, 10], [40, 40, 50, 50]], [0.7, 0.9, 0.8])
    r = L.evaluate([im], 1, [0.5], ALL)
    assert r['flags'][0][:, 0].tolist() == [1, 1, 0] and r['ranks'][0].tolist() == [2, 0, 1]
    for k in ('ap', 'ap_mean'):
        assert abs(r[k][0, 0, 0, 0] - (51 + 50 * 2 / 3) / 101) < 1e-13
    assert r['ar'][0, 0, 0, 0] == 1.0


# ------------------------------------------------------------------------------------------------ against the COCO restatement
@pytest.mark.parametrize('seed,C,M,n_det', [(1, 3, 12, 30), (2, 5, 40, 60), (3, 2, 6, 25)])
def test_equals_the_coco_restatement_where_the_protocols_coincide(seed, C, M, n_det):
    """neg = all categories, no nel, no crowd, rows in descending score order, at most max_dets[-1] detections an image: flag
    words, npig, precision, AP and AR equal tests/_coco_eval_ref.py bit for bit.  (The stored ranks differ by definition: the
    rank in the image here, the rank in the class there; both stay below max_dets[-1], so neither acts.)"""
    images = K.random_images(seed, 4, C, M, n_det, crowd_frac=0.0, scores_levels=16 if seed == 2 else 0)
    for im in images:
        im['neg'], im['nel'] = list(range(C)), None
    md = (n_det,)
    a, b = L.evaluate(images, C, max_dets=md), K.evaluate(images, C, max_dets=md)
    for x, y in zip(a['flags'], b['flags']):
        assert np.array_equal(x, y)
    assert np.array_equal(a['npig'], b['npig']) and np.array_equal(a['scores'], b['scores']) and np.array_equal(a['words'], b['words'])
    for k in ('precision', 'ap', 'ap_mean', 'ar'):
        assert _same(a[k], b[k]), k
    assert np.nanmax(a['ap']) > 0 and all((x < n_det).all() and (y < n_det).all() for x, y in zip(a['ranks'], b['ranks']))
    assert np.array_equal(L.sorted_entries(a['scores'], a['classes'], C), K.sorted_entries(b['scores'], b['classes'], C))


def test_random_cases_contain_every_rule():
    images = L.random_images(5, 4, 6, 12, 40, scores_levels=16)
    st = L.evaluate(images, 6, max_dets=(25,))['stats']
    assert st['cut'] > 0 and st['filtered'] > 0 and st['nel'] > 0, st


def test_against_lvis_api_where_installed(tmp_path):
    lvis = pytest.importorskip('lvis')
    C = 4
    images = L.random_images(7, 6, C, 10, 30, grid=8.0, size=80.0)
    near = lambda im, d: any(abs(float(L._iou(d, g)) - t) <= 1e-6 for g in im['gt_boxes'] for t in L.LVIS_THRESHOLDS)
    for im in images:                                                         # float32 and float64 IoU must decide alike
        keep = np.array([0 <= c < C and not near(im, d) for d, c in zip(im['det_boxes'], im['det_classes'])], bool)
        for k in ('det_boxes', 'det_scores', 'det_classes'):
            im[k] = im[k][keep]
        im['neg'] = [c for c in im['neg'] if c not in set(im['gt_classes'].tolist())]      # LVIS keeps pos and neg disjoint
    freq = ['r', 'c', 'f', 'c']
    anns, dets, k = [], [], 1
    for i, im in enumerate(images):
        for b, c in zip(im['gt_boxes'], im['gt_classes']):
            w, h = float(b[3] - b[1]), float(b[2] - b[0])
            anns.append(dict(id=k, image_id=i + 1, category_id=int(c) + 1, bbox=[float(b[1]), float(b[0]), w, h], area=w * h,
                             segmentation=[[float(b[1]), float(b[0]), float(b[3]), float(b[0]), float(b[3]), float(b[2])]]))
            k += 1
        for b, s, c in zip(im['det_boxes'], im['det_scores'], im['det_classes']):
            dets.append(dict(image_id=i + 1, category_id=int(c) + 1, score=float(s),
                             bbox=[float(b[1]), float(b[0]), float(b[3] - b[1]), float(b[2] - b[0])]))
    gt = dict(images=[dict(id=i + 1, height=200, width=200, neg_category_ids=[c + 1 for c in im['neg']],
                           not_exhaustive_category_ids=[c + 1 for c in im['nel']]) for i, im in enumerate(images)],
              annotations=anns, categories=[dict(id=c + 1, name='c%d' % c, frequency=freq[c]) for c in range(C)])
    path = tmp_path / 'gt.json'
    path.write_text(json.dumps(gt))
    api = lvis.LVIS(str(path))
    E = lvis.LVISEval(api, lvis.LVISResults(api, dets, max_dets=20), 'bbox')
    E.params.max_dets = 20
    E.run()
    r = L.evaluate(images, C, max_dets=(20,))
    want = np.where(E.eval['precision'] < 0, np.nan, E.eval['precision'])
    assert np.allclose(r['precision'][..., 0], want, rtol=0, atol=1e-12, equal_nan=True)
    got = L.summarize(r['ap_mean'], r['ar'], freq)
    names = ('AP', 'AP50', 'AP75', 'APs', 'APm', 'APl', 'APr', 'APc', 'APf', 'AR@20', 'ARs@20', 'ARm@20', 'ARl@20')
    assert np.allclose(got, [E.results[n] for n in names], rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------------ C ABI
P = 0x1000                                                                   # a non-null pointer that is never dereferenced


def _lib():
    from ood_object_detection_amd import _lib
    return _lib.load()


def check_abi_refusals(lib):
    def match(thr=(0.5,), T=None, areas=((0, 1e10),), A=None, C=5, B=2, max_det=10, M=4, max_rank=300, min_score=0.0, Kn=3, Ke=3, **null):
        p = dict(det=P, cnt=P, gtb=P, gtc=P, neg=P, nel=P, flags=P, rank=P, npig=P)
        p.update(null)
        t = (ctypes.c_float * max(len(thr), 1))(*thr)
        ar = (ctypes.c_float * max(2 * len(areas), 2))(*[v for r in areas for v in r])
        return lib.effdet_lvis_match(None, p['det'], p['cnt'], p['gtb'], p['gtc'], None, B, max_det, M, C, t,
                                     len(thr) if T is None else T, ar, len(areas) if A is None else A, max_rank, min_score,
                                     p['neg'], Kn, p['nel'], Ke, p['flags'], p['rank'], P, p['npig'])
    assert match(thr=()) == -22 and match(thr=[0.5] * 15, T=16) == -22
    assert match(thr=[0.5, 0.5]) == -22 and match(thr=[0.75, 0.5]) == -22 and match(thr=[0.5, float('nan')]) == -22
    assert match(areas=()) == -22 and match(areas=[(0, 1)] * 4, A=5) == -22 and match(areas=[(2, 1)]) == -22
    assert match(areas=[(float('nan'), 1)]) == -22
    for name in ('det', 'cnt', 'gtb', 'gtc', 'flags', 'rank', 'npig'):
        assert match(**{name: None}) == -22, name
    assert match(C=0) == -22 and match(C=65536) == -22
    assert match(B=0) == -22 and match(max_det=0) == -22 and match(M=0) == -22 and match(B=1 << 20, max_det=17) == -22
    assert match(max_det=2049, B=1) == -22                                                             # beyond the max_det limit
    assert match(M=1640) == -22 and match(M=1300, max_det=2048, B=1) == -22 and match(M=1500, C=65535) == -22      # > 64 KiB of LDS
    assert match(max_rank=0) == -22 and match(min_score=float('nan')) == -22
    assert match(Kn=-1) == -22 and match(Ke=-1) == -22


def test_abi_refusals():
    check_abi_refusals(_lib())


def test_lds_query():
    lib = _lib()
    assert lib.effdet_lvis_match_lds_bytes(300, 16, 1203) == 40 * 16 + 12 * 38 + 8 * 300 + 16
    assert lib.effdet_lvis_match_lds_bytes(1, 1, 32) == 40 + 12 + 8 + 16 and lib.effdet_lvis_match_lds_bytes(1, 1, 33) == 40 + 24 + 8 + 16
    assert lib.effdet_lvis_match_lds_bytes(2048, 1, 1) > 0 and lib.effdet_lvis_match_lds_bytes(1024, 300, 1203) <= 64 * 1024
    for bad in ((0, 16, 80), (2049, 16, 80), (300, 0, 80), (300, 16, 0), (300, 16, 65536)):
        assert lib.effdet_lvis_match_lds_bytes(*bad) == -22


def test_header_exports_and_ctypes_table_agree():
    from ood_object_detection_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'effdet_hip.h')).read()
    declared = set(re.findall(r'\b(effdet_lvis_[a-z0-9_]+)\s*\(', header))
    assert declared == {'effdet_lvis_match', 'effdet_lvis_match_lds_bytes'}
    assert declared == {n for n in _lib.SIGNATURES if n.startswith('effdet_lvis_')}
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name), name
    proto = re.search(r'int effdet_lvis_match\((.*?)\);', header, re.S).group(1)
    assert len(proto.split(',')) == len(_lib.SIGNATURES['effdet_lvis_match'][1]) == 24


# ------------------------------------------------------------------------------------------------ Python
def test_python_api_argument_checks():
    from ood_object_detection_amd.effdet.evaluation import CocoDetectionEvaluator, LvisDetectionEvaluator
    assert issubclass(LvisDetectionEvaluator, CocoDetectionEvaluator)
    cats = [{'id': 1, 'name': 'a', 'frequency': 'r'}]
    with pytest.raises(RuntimeError):
        LvisDetectionEvaluator(cats, device='cpu')                            # no CPU fallback
    for kw in (dict(iou_thresholds=()), dict(area_ranges=[(2, 1)]), dict(max_dets=()), dict(max_dets=(0,)), dict(max_dets=(300, 300)),
               dict(recall_thresholds=(0.5, 0.25)), dict(min_score=float('nan')), dict(capacity=0), dict(capacity=(1 << 24) + 1)):
        with pytest.raises(ValueError):
            LvisDetectionEvaluator(cats, device='cpu', **kw)
    with pytest.raises(ValueError):
        LvisDetectionEvaluator([{'id': 0, 'name': 'a'}])


def _lvis_dict():
    return dict(
        images=[dict(id=11, neg_category_ids=[5, 2], not_exhaustive_category_ids=[9]), dict(id=7, neg_category_ids=[], not_exhaustive_category_ids=[]),
                dict(id=3, neg_category_ids=[9, 77])],
        annotations=[dict(image_id=11, bbox=[10, 20, 30, 40], area=600.0, category_id=9), dict(image_id=3, bbox=[1, 2, 3, 4], category_id=2),
                     dict(image_id=11, bbox=[0, 0, 5, 5], area=20.0, category_id=5), dict(image_id=11, bbox=[0, 0, 1, 1], area=1.0, category_id=77),
                     dict(image_id=99, bbox=[0, 0, 1, 1], area=1.0, category_id=2)],
        categories=[dict(id=2, name='two', frequency='r'), dict(id=5, name='five', frequency='c'), dict(id=9, name='nine', frequency='f')])


def test_lvis_ground_truth():
    from ood_object_detection_amd.effdet.evaluator import lvis_ground_truth
    g = lvis_ground_truth(_lvis_dict())
    assert g['img_ids'] == [11, 7, 3] and tuple(g['gt_boxes'].shape) == (3, 2, 4)
    assert g['gt_boxes'][0].tolist() == [[20, 10, 60, 40], [0, 0, 5, 5]] and g['gt_boxes'][2, 0].tolist() == [2, 1, 6, 4]
    assert g['gt_cls'].tolist() == [[9, 5], [-1, -1], [2, -1]]                # category 77 is not in `categories`: left out
    assert g['gt_area'].tolist() == [[600, 20], [0, 0], [12, 0]]              # `area` as given (not w * h = 1200); w * h without one
    assert g['neg_cls'].tolist() == [[5, 2], [-1, -1], [9, -1]] and g['nel_cls'].tolist() == [[9], [-1], [-1]]
    assert g['categories'] == [dict(id=2, name='two', frequency='r'), dict(id=5, name='five', frequency='c'), dict(id=9, name='nine', frequency='f')]
    g = lvis_ground_truth(_lvis_dict(), cat_id_to_label={2: 1, 5: 2, 9: 3}, M=4, Kn=3, Ke=2)
    assert tuple(g['gt_boxes'].shape) == (3, 4, 4) and g['gt_cls'][0].tolist() == [3, 2, -1, -1]
    assert g['neg_cls'].tolist() == [[2, 1, -1], [-1, -1, -1], [3, -1, -1]] and tuple(g['nel_cls'].shape) == (3, 2)
    assert [c['id'] for c in g['categories']] == [1, 2, 3]
    for kw in (dict(M=1), dict(Kn=1), dict(cat_id_to_label={2: 0, 5: 1, 9: 2})):
        with pytest.raises(ValueError):
            lvis_ground_truth(_lvis_dict(), **kw)
    d = _lvis_dict()
    for c in d['categories']:
        del c['frequency']
    assert all('frequency' not in c for c in lvis_ground_truth(d)['categories'])


def test_create_evaluator_still_mirrors_the_reference_dispatch():
    from ood_object_detection_amd.effdet import evaluator as E
    assert 'LvisEvaluator' in E.__all__ and 'lvis_ground_truth' in E.__all__
    ev = E.LvisEvaluator(_lvis_dict(), device='cuda:0')                       # nothing touches the device before the first batch
    assert ev._dataset.img_ids == [11, 7, 3]
    with pytest.raises(ValueError):
        E.LvisEvaluator(dict(images=[], annotations=[], categories=[]))
