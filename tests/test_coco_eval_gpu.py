"""csrc/coco_eval.hip on the device (-m gpu): COCO-protocol matching (crowd regions, area ranges, ties, ranks), the append, the
sort with the entry index as payload, AP / AR / precision and the evaluators on top, against tests/_coco_eval_ref.py and against
themselves (bit-identical runs).

Flag words, ranks, npig and the sorted order are compared EXACTLY: both sides compute the IoU by the same float32 operations.
precision, AP and AR are compared BITWISE with the restatement's sequential sum: every term is one float64 division and AP is R
additions in ascending r on both sides.  Against the np.mean form (pairwise summation) the bound is derived: each side adds R
terms q[r] in [0, 1], every partial sum is <= R and is rounded once (relative 2^-53), so each sum is within R * R * 2^-53 of the
exact one and each mean within R * 2^-53; the two differ by at most 2 R 2^-53 (4.5e-14 for R = 101; 1.1e-13 for R = 256)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _coco_eval_ref as K
from test_coco_eval_host import _Dataset, _Parser, _im, check_abi_refusals

DEV = 'cuda:0'
F = np.float32


def _cats(C):
    return [{'id': i + 1, 'name': 'c%d' % i} for i in range(C)]


def _evaluator(C, **kw):
    from ood_object_detection_amd.effdet.evaluation import CocoDetectionEvaluator
    return CocoDetectionEvaluator(_cats(C), device=DEV, **kw)


def _pack(images, max_det, M):
    return [torch.from_numpy(a).to(DEV) if a is not None else None for a in K.pack(images, max_det, M)]


def _bits(a):
    a = np.asarray(a, np.float64)
    return np.isnan(a), np.where(np.isnan(a), 0.0, a).view(np.uint64)


def _assert_bitwise(got, ref, what):
    (gn, gb), (rn, rb) = _bits(got), _bits(ref)
    assert got.shape == ref.shape and np.array_equal(gn, rn), what
    assert np.array_equal(gb, rb), (what, np.abs(np.nan_to_num(got) - np.nan_to_num(ref)).max())


def _assert_mean_form(ap, ap_mean, R):
    err = np.abs(np.nan_to_num(ap) - np.nan_to_num(ap_mean)).max()
    print('AP against the np.mean form: error', err, 'bound', 2 * R * 2.0 ** -53)
    assert err <= 2 * R * 2.0 ** -53


def _check(images, C, M, max_det, splits=1, **kw):
    """the evaluator on `images` against the restatement: everything, exactly"""
    ev = _evaluator(C, capacity=len(images) * max_det + 7, keep_precision=True, **kw)
    ref = K.evaluate(images, C, kw.get('iou_thresholds', K.COCO_THRESHOLDS), kw.get('area_ranges', K.COCO_AREAS),
                     kw.get('max_dets', K.COCO_MAX_DETS), kw.get('recall_thresholds', K.COCO_REC_THRS), kw.get('min_score', 0.0))
    flags, ranks = [], []
    for idx in np.array_split(np.arange(len(images)), splits):
        flags.append(ev.add_batch(*_pack([images[i] for i in idx], max_det, M)).cpu().numpy().view(np.uint32))
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
    assert r['n'] == n and r['lost'] == 0 and r['nan_scores'] == ref['nan_scores']
    assert np.array_equal(r['npig'], ref['npig'])
    cls, scores, words, rk, index = ev.sorted()
    order = K.sorted_entries(ref['scores'], ref['classes'], C)
    assert np.array_equal(index, order) and np.array_equal(cls, ref['classes'][order]) and np.array_equal(scores, ref['scores'][order] + F(0))
    assert np.array_equal(words, ref['words'][order]) and np.array_equal(rk, ref['rank'][order])
    _assert_bitwise(ev.precision().cpu().numpy(), ref['precision'], 'precision')
    _assert_bitwise(r['ap'], ref['ap'], 'AP')
    _assert_bitwise(r['ar'], ref['ar'], 'AR')
    _assert_mean_form(r['ap'], ref['ap_mean'], len(kw.get('recall_thresholds', K.COCO_REC_THRS)))
    return ref


# ------------------------------------------------------------------------------------------------ matching
def _special_images():
    return [
        _im([[0, 0, 100, 100], [200, 200, 210, 210]], [0, 0], [[200, 200, 210, 210], [10, 10, 20, 20], [50, 50, 80, 80]],
            [0.9, 0.8, 0.7], gt_crowd=[True, False]),                                      # a crowd region absorbs two detections
        _im([[0, 0, 32, 32], [100, 100, 196, 196], [0, 0, 10, 10]], [1, 1, 1], [[0, 0, 32, 32], [100, 100, 196, 196], [300, 300, 332, 332]],
            [0.9, 0.8, 0.7], det_cls=[1, 1, 1], gt_area=[1024.0, 9216.0, 9217.0]),         # areas on the edges of the ranges
        _im([[0, 0, 10, 10], [0, 10, 10, 20]], [0, 0], [[0, 0, 10, 20], [0, 0, 10, 10], [0, 10, 10, 20]], [0.9, 0.8, 0.7]),      # a tie
        _im([[0, 0, 10, 40], [100, 0, 110, 40]], [2, 2], [[0, 0, 10, 30], [100, 0, 110, 20]], [0.9, 0.8], det_cls=[2, 2]),    # IoU .75, .5
        _im(np.zeros((0, 4)), [], [[0, 0, 10, 10], [0, 0, 20, 20]], [0.5, 0.25], det_cls=[0, 2]),      # no boxes
        _im([[0, 0, 10, 10], [0, 0, 50, 50]], [0, 1], np.zeros((0, 4)), []),                           # no detections
        _im([[0, 0, 10, 10], [0, 0, 10, 10]], [0, 0], [[0, 0, 10, 10]] * 4, [0.9, 0.9, 0.5, np.nan], gt_crowd=[False, True]),
    ]


@pytest.mark.parametrize('params', [dict(), dict(iou_thresholds=[0.5], area_ranges=[K.COCO_AREAS[0]], max_dets=[100]),
                                    dict(iou_thresholds=np.linspace(0.25, 0.95, 15))], ids=['T10_A4', 'T1_A1', 'T15'])
def test_special_cases(params):
    ref = _check(_special_images(), 3, 3, 5, splits=2, **params)
    f = ref['flags']
    T = len(params.get('iou_thresholds', K.COCO_THRESHOLDS))
    assert (f[0][1:, 0] >> 16).all() and not (f[0][1:, 0] & 0xFFFF).any()                 # ignored by the crowd region, never a TP
    assert [int(w) & 1 for w in f[2][:, 0]] == [1, 1, 0]                                  # the tie went to the later box
    if T == 10:
        assert f[3][:, 0].tolist() == [0b111111, 0b1] and ref['npig'][1].tolist() == [4, 1, 3, 2]      # 1024 / 9216 lie in two ranges


@pytest.mark.parametrize('M,max_det,n_det', [(1, 100, 40), (255, 100, 100), (257, 100, 60), (300, 300, 300)])
def test_matching_sizes(M, max_det, n_det):
    C = 5
    images = K.random_images(100 + M, 2, C, M, n_det, scores_levels=32 if M == 257 else 0)
    images[0]['gt_area'] = (K.box_area(images[0]['gt_boxes']) * F(0.75)).astype(F)       # segmentation area, not the box area
    images[1]['gt_area'] = K.box_area(images[1]['gt_boxes'])
    ref = _check(images, C, M, max_det)
    words = np.concatenate(ref['flags'])
    assert (words & 0x3FF).any() and ((words >> 16) & 0x3FF).any() and (words >> 31).any()


def test_images_in_any_split_give_the_same_bits_and_runs_repeat():
    C, M, max_det = 4, 40, 50
    images = K.random_images(9, 9, C, M, max_det, scores_levels=16)
    ev = _evaluator(C, capacity=4096, keep_precision=True)

    def run(e, parts):
        e.clear()
        for idx in np.array_split(np.arange(len(images)), parts):
            e.add_batch(*_pack([images[i] for i in idx], max_det, M))
        e.enqueue()
        return e.result()['block'], e.precision().cpu().numpy().copy()
    blocks = [run(ev, parts) for parts in (1, 3, 9, 1)]
    blocks.append(run(_evaluator(C, capacity=1 << 16, keep_precision=True), 2))
    for b, p in blocks[1:]:
        assert np.array_equal(b, blocks[0][0]) and np.array_equal(_bits(p)[1], _bits(blocks[0][1])[1])
    ref = K.evaluate(images, C)
    _assert_bitwise(blocks[0][0][8:8 + ref['ap'].size].view(np.float64).reshape(ref['ap'].shape), ref['ap'], 'AP')


# ------------------------------------------------------------------------------------------------ accumulate
def _load_entries(ev, scores, classes, words, ranks, npig):
    n = len(scores)
    ev.clear()
    ev._bufs[0][:n] = torch.from_numpy(scores).to(DEV)
    ev._bufs[1][:n] = torch.from_numpy(classes.astype(np.int32)).to(DEV)
    ev._bufs[2][:words.size] = torch.from_numpy(words.astype(np.uint32).view(np.int32).reshape(-1)).to(DEV)
    ev._bufs[3][:n] = torch.from_numpy(ranks.astype(np.int32)).to(DEV)
    ev._state[0] = n
    ev._npig.copy_(torch.from_numpy(npig.astype(np.int32).reshape(-1)).to(DEV))


def _random_entries(seed, sizes, T, A):
    """classes of the given sizes (class k: sizes[k] entries, shuffled over the arrival order), scores on a 1/64 grid (ties across
    the whole set), words with TP / ignored bits, ranks 0 .. 119"""
    rs = np.random.RandomState(seed)
    classes = rs.permutation(np.repeat(np.arange(len(sizes)), sizes))
    n = len(classes)
    scores = (rs.randint(0, 65, n) / F(64)).astype(F)
    mask = (1 << T) - 1
    words = ((rs.randint(0, 1 << T, (n, A)) & rs.randint(0, 1 << T, (n, A))) & mask).astype(np.uint32)
    ign = (rs.randint(0, 1 << T, (n, A)) & rs.randint(0, 1 << T, (n, A)) & rs.randint(0, 1 << T, (n, A))) & mask
    words = (words & ~ign.astype(np.uint32)) | (ign.astype(np.uint32) << np.uint32(16))
    ranks = np.minimum(rs.randint(0, 120, n), rs.randint(0, 120, n)).astype(np.int32)
    return scores, classes, words, ranks


@pytest.mark.parametrize('sizes,T,A', [((1, 2047, 2047, 0, 0), 2, 2), ((1, 2047, 2048, 0, 0), 2, 2), ((2048, 2049, 0, 0, 0), 10, 4),
                                       ((1, 2047, 2048, 2049, 5), 3, 1)], ids=['4095', '4096', '4097', '6150'])
def test_accumulate_segments_and_sort_tiles(sizes, T, A):
    """segments of 1 / 2047 / 2048 / 2049 entries (the AP chunk is 2048) in totals of 4095 / 4096 / 4097 (the sort tile is 4096);
    npig 4, 10, 20, 50, 100 (k / npig meets recall thresholds exactly); a class with npig and no entry; a class with entries and
    npig 0"""
    C = len(sizes)
    scores, classes, words, ranks = _random_entries(sum(sizes), sizes, T, A)
    npig = np.array([[(4, 10, 20, 50, 100)[(c + a) % 5] for a in range(A)] for c in range(C)], np.int64)
    npig[C - 1] = 0 if sizes[C - 1] else npig[C - 1]                                      # entries without boxes -> NaN
    thr = np.linspace(0.5, 0.95, 10)[:T]
    ev = _evaluator(C, iou_thresholds=thr, area_ranges=K.COCO_AREAS[:A], capacity=sum(sizes) + 3, keep_precision=True)
    _load_entries(ev, scores, classes, words, ranks, npig)
    ev.enqueue()
    r = ev.result()
    ref = K.accumulate(scores, classes, words, ranks, npig, C, T)
    assert r['n'] == sum(sizes) and np.array_equal(r['npig'], npig)
    index = ev.sorted()[4]
    assert np.array_equal(index, K.sorted_entries(scores, classes, C))
    _assert_bitwise(ev.precision().cpu().numpy(), ref['precision'], 'precision')
    _assert_bitwise(r['ap'], ref['ap'], 'AP')
    _assert_bitwise(r['ar'], ref['ar'], 'AR')
    _assert_mean_form(r['ap'], ref['ap_mean'], 101)
    assert np.nanmax(r['ap']) > 0.01 and (np.isnan(r['ap'][:, C - 1]).all() if sizes[C - 1] else True)
    empty = [c for c in range(C) if sizes[c] == 0]
    assert all((r['ap'][:, c] == 0).all() and (r['ar'][:, c] == 0).all() for c in empty)      # boxes, no detection: 0, not NaN


def test_recall_table_of_256_entries_and_one_entry():
    scores, classes, words, ranks = _random_entries(5, (300, 40), 2, 1)
    npig = np.array([[50], [7]], np.int64)
    for rec in (np.linspace(0, 1, 256), np.array([0.5]), np.array([0.0, 0.02, 0.02 + 2.0 ** -50, 1.0, 1.5])):
        ev = _evaluator(2, iou_thresholds=[0.5, 0.75], area_ranges=[K.COCO_AREAS[0]], recall_thresholds=rec, capacity=512, keep_precision=True)
        _load_entries(ev, scores, classes, words, ranks, npig)
        ev.enqueue()
        ref = K.accumulate(scores, classes, words, ranks, npig, 2, 2, rec_thr=rec)
        _assert_bitwise(ev.precision().cpu().numpy(), ref['precision'], 'precision')
        _assert_bitwise(ev.result()['ap'], ref['ap'], 'AP')


# ------------------------------------------------------------------------------------------------ mechanics
def test_add_batch_and_enqueue_in_a_captured_graph():
    C, M, max_det = 4, 40, 50
    images = K.random_images(21, 6, C, M, max_det)
    ev = _evaluator(C, capacity=4096)
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
    assert eager[0] > 100


def test_overflow_is_reported_and_clear_allows_reuse():
    C, M, max_det = 3, 8, 100
    images = K.random_images(31, 12, C, M, max_det)
    for im in images:
        im['det_classes'] = np.clip(im['det_classes'], 0, C - 1)
    total = sum(int((K.kept_ranks(im, C, 100) >= 0).sum()) for im in images)
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
    ref = K.evaluate(images[:5], C)
    assert r['n'] == len(ref['scores']) and r['lost'] == 0
    _assert_bitwise(r['ap'], ref['ap'], 'AP')


def test_min_score_drops_detections_before_they_are_ranked():
    C, M, max_det = 3, 30, 60
    images = K.random_images(41, 3, C, M, max_det, scores_levels=20)
    ref = _check(images, C, M, max_det, min_score=0.35, max_dets=(1, 5, 10))
    assert all((r[im['det_scores'] < F(0.35)] == -1).all() for r, im in zip(ref['ranks'], images))
    assert max(r.max() for r in ref['ranks']) == 9                                        # and the ranks stop at max_dets[-1]


def test_abi_refusals_with_the_device_present():
    from ood_object_detection_amd import _lib
    check_abi_refusals(_lib.load())
    ev = _evaluator(2, capacity=16)
    with pytest.raises(ValueError):
        ev.add_batch(torch.zeros(2, 4, 5), torch.zeros(2), torch.zeros(2, 1, 4), torch.zeros(2, 1))
    with pytest.raises(ValueError):
        ev.add_batch(torch.zeros(2, 4, 6), torch.zeros(2), torch.zeros(2, 1, 4), torch.zeros(2, 1), gt_crowd=torch.zeros(2, 2))
    with pytest.raises(RuntimeError):
        ev.add_batch(torch.zeros(1, 4, 6), torch.zeros(1), torch.zeros(1, 1700, 4), torch.zeros(1, 1700))       # LDS: -22
    with pytest.raises(RuntimeError):
        ev.precision()


# ------------------------------------------------------------------------------------------------ the evaluators on top
def test_evaluate_names_the_twelve_coco_figures():
    C = 4
    images = K.random_images(51, 8, C, 20, 40)
    ev = _evaluator(C, capacity=1024)
    ev.add_batch(*_pack(images, 40, 20))
    out = ev.evaluate()
    ref = K.evaluate(images, C)
    want = K.summarize(ref['ap'], ref['ar'])
    assert np.array_equal(out['stats'], want) and np.array_equal(ev.stats, want)
    keys = [k for k in out if '@[' in k]
    assert keys[0] == 'AP@[IoU=0.50:0.95|area=all|maxDets=100]' and keys[1] == 'AP@[IoU=0.50|area=all|maxDets=100]'
    assert keys[5] == 'AP@[IoU=0.50:0.95|area=large|maxDets=100]' and keys[6] == 'AR@[IoU=0.50:0.95|area=all|maxDets=1]'
    assert len(keys) == 12 and [out[k] for k in keys] == want.tolist() and want[0] > 0
    per_class = np.array([out['AP/c%d' % c] for c in range(C)])
    assert np.allclose(np.nanmean(per_class), want[0], rtol=0, atol=1e-12)


def _synthetic_dataset(C=3, M=12, max_det=30):
    """7 images with crowd boxes and an annotation `area` of half the box area, as a parser of plain data (image ids 100 ..);
    -> (images, dataset, det [7, max_det + 3, 6] with rows of zeros behind the detections)"""
    images = K.random_images(61, 7, C, M, max_det, crowd_frac=0.2)
    anns = {}
    for i, im in enumerate(images):
        area = K.box_area(im['gt_boxes']) * F(0.5)
        im['gt_area'] = area
        anns[100 + i] = [dict(bbox=[float(b[1]), float(b[0]), float(b[3] - b[1]), float(b[2] - b[0])], category_id=int(c) + 1,
                              iscrowd=int(cr), area=float(a)) for b, c, cr, a in zip(im['gt_boxes'], im['gt_classes'], im['gt_crowd'], area)]
    return images, _Dataset(_Parser(anns, list(range(1, C + 1)))), torch.from_numpy(K.pack(images, max_det + 3, M)[0])


def test_coco_evaluator_end_to_end_on_a_synthetic_parser(tmp_path):
    from ood_object_detection_amd.effdet.evaluator import create_evaluator
    C = 3
    images, ds, det = _synthetic_dataset(C)
    ev = create_evaluator('coco', ds, keep_predictions=True, device=DEV)
    for idx in ([4, 0, 6], [1, 5], [3, 2]):                                               # any order of the images
        ev.add_predictions(det[idx].to(DEV), dict(img_idx=torch.tensor(idx, device=DEV)))
    path = tmp_path / 'results.json'
    ev.save(str(path))
    metric = ev.evaluate()
    ref = K.evaluate([images[i] for i in (4, 0, 6, 1, 5, 3, 2)], C, min_score=0.001)
    want = K.summarize(ref['ap'], ref['ar'])
    assert metric == want[0] and np.array_equal(ev.metrics['stats'], want) and metric > 0
    import json
    rows = json.loads(path.read_text())
    assert len(rows) == sum(int((im['det_scores'] >= F(0.001)).sum()) for im in images) and rows[0]['image_id'] == 104
    assert ev.predictions == [] and int(ev._evaluator._state[0]) == 0                     # evaluate() resets
    yx = create_evaluator('coco', ds, pred_yxyx=True, device=DEV)
    for idx in ([4, 0, 6], [1, 5], [3, 2]):
        yx.add_predictions(det[idx][:, :, [1, 0, 3, 2, 4, 5]].to(DEV), dict(img_idx=torch.tensor(idx)))
    assert yx.evaluate() == metric


def test_coco_evaluator_distributed_path_in_a_world_of_one(tmp_path):
    """distributed=True: barrier, all_gather_container of detections and indices, rank 0 evaluates, the metric is broadcast"""
    import torch.distributed as dist
    from ood_object_detection_amd.effdet.evaluator import create_evaluator
    images, ds, det = _synthetic_dataset()
    plain = create_evaluator('coco', ds, device=DEV)
    plain.add_predictions(det.to(DEV), dict(img_idx=torch.arange(7, device=DEV)))
    want = plain.evaluate()
    own = not dist.is_initialized()
    if own:
        dist.init_process_group('gloo', init_method='file://' + str(tmp_path / 'store'), rank=0, world_size=1)
    try:
        ev = create_evaluator('coco', ds, distributed=True, device=DEV)
        for idx in ([0, 1, 2, 3], [4, 5, 6]):
            ev.add_predictions(det[idx].to(DEV), dict(img_idx=torch.tensor(idx, device=DEV)))
        assert ev.evaluate() == want and want > 0
    finally:
        if own:
            dist.destroy_process_group()


def test_pascal_evaluator_runs_on_the_device_evaluator():
    from ood_object_detection_amd.effdet.evaluation import PascalDetectionEvaluator
    from ood_object_detection_amd.effdet.evaluator import create_evaluator
    C, M, max_det = 3, 6, 20
    images = K.random_images(71, 4, C, M, max_det, crowd_frac=0.0)
    parser = _Parser({i: [] for i in range(len(images))}, [1, 2, 3])
    parser.get_ann_info = lambda i: dict(bbox=images[i]['gt_boxes'], cls=images[i]['gt_classes'] + 1)
    ev = create_evaluator('voc', _Dataset(parser), device=DEV)
    det, cnt, gtb, gtc, _, _ = _pack(images, max_det, M)
    ev.add_predictions(det, dict(img_idx=torch.arange(len(images))))
    direct = PascalDetectionEvaluator(parser.cat_dicts, device=DEV)
    direct.add_batch(det, cnt, gtb, gtc)
    want = direct.evaluate()['PascalBoxes_Precision/mAP@0.5IOU']
    assert ev.evaluate() == want and want > 0


def test_detbench_predict_batch_feeds_the_evaluator():
    """one tf_efficientdet_d0 batch at 128 px: detections and counts go from DetBenchPredict to add_batch as device tensors; the
    ground truth is made of the images' own top detections (on the device), so true positives exist"""
    from _models import seeded_model
    from _seeded import seeded_array
    from ood_object_detection_amd.effdet.bench import DetBenchPredict
    model, cfg, _, _ = seeded_model('tf_efficientdet_d0', 128, 20, seed=11)
    bench = DetBenchPredict(model.to(DEV).float()).to(DEV)
    det = bench(torch.from_numpy(seeded_array(11, 'input', (2, 3, 128, 128))).to(DEV))
    count = bench.last_count
    gt_boxes = det[:, :6, [1, 0, 3, 2]].contiguous()
    gt_cls = det[:, :6, 5].to(torch.int64)
    gt_crowd = torch.zeros(2, 6, dtype=torch.uint8, device=DEV)
    gt_crowd[:, 5] = 1
    ev = _evaluator(20, capacity=512, min_score=0.001)
    flags = ev.add_batch(det, count, gt_boxes, gt_cls, gt_crowd)
    ev.enqueue()
    r = ev.result()                                                                       # the first host read
    d, n = det.cpu().numpy(), count.cpu().numpy()
    images = [dict(det_boxes=d[b, :n[b]][:, [1, 0, 3, 2]], det_scores=d[b, :n[b], 4], det_classes=d[b, :n[b], 5].astype(np.int64) - 1,
                   gt_boxes=d[b, :6][:, [1, 0, 3, 2]], gt_classes=d[b, :6, 5].astype(np.int64) - 1, gt_crowd=[0, 0, 0, 0, 0, 1]) for b in range(2)]
    ref = K.evaluate(images, 20, min_score=0.001)
    f = flags.cpu().numpy().view(np.uint32)
    for b in range(2):
        assert np.array_equal(f[b, :n[b]], ref['flags'][b]) and (f[b, n[b]:] == 0x80000000).all()
    _assert_bitwise(r['ap'], ref['ap'], 'AP')
    _assert_bitwise(r['ar'], ref['ar'], 'AR')
    assert np.nanmax(r['ap']) > 0.5 and r['n'] == len(ref['scores']) > 0
