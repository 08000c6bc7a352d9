"""csrc/openimages_eval.hip on the device (-m gpu): the two-stage matching with group-of boxes, the virtual entries, the verified
labels, the append, both sorts, the weighted AP and the pooled AP, against tests/_eval_openimages_ref.py (pinned to the reference's
evaluators by tests/golden/evaluation_openimages.npz), against DatasetDetectionEvaluator where the two protocols coincide, and
against themselves (splits, a captured graph).

Flag words, virtual entries, kept counts, counters and both sorted orders are compared EXACTLY; AP and pooled AP BITWISE: the
restatement adds in the kernel's order.  Against the fixture (the reference's own order of the same sum) the bound is 1e-12, the
yardstick of tests/test_eval_scale_gpu.py."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _eval_openimages_ref as O

DEV = 'cuda:0'
INVALID = 0x80000000
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cats(C):
    return [{'id': i + 1, 'name': 'c%d' % i} for i in range(C)]


def _evaluator(C, thresholds=(0.5,), w=0.0, cls=None, **kw):
    from ood_object_detection_amd.effdet.evaluation import OpenImagesDetectionEvaluator
    return (cls or OpenImagesDetectionEvaluator)(_cats(C), iou_thresholds=thresholds, group_of_weight=w, device=DEV, **kw)


def _golden():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'evaluation_openimages.npz'))


def _pack(images, max_det, M, K=None):
    """(det, count, gt_boxes, gt_cls) and dict(gt_group_of, gt_difficult, labeled_cls) on the device"""
    det, cnt, gtb, gtc, gtd, gtg, lab = O.pack(images, max_det, M, K)
    t = lambda a: torch.from_numpy(a).to(DEV)
    return (t(det), t(cnt), t(gtb), t(gtc)), dict(gt_group_of=t(gtg), gt_difficult=t(gtd), labeled_cls=t(lab) if lab is not None else None)


def _u32(t):
    return t.cpu().numpy().astype(np.int64) & 0xFFFFFFFF


def _same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.array_equal(np.where(np.isnan(a), 0.0, a).view(np.uint64), np.where(np.isnan(b), 0.0, b).view(np.uint64))


# ------------------------------------------------------------------------------------------------ matching
# M on both sides of the 256-thread staging loop (the second trip starts above 256); no, some and only group-of boxes; T = 1, 3, 15
MATCH_CASES = [(1, 1.0, 1, None), (1, 0.0, 3, None), (64, 0.3, 3, 2), (64, 1.0, 15, None), (257, 0.3, 15, None), (257, 0.0, 1, 1),
               (300, 0.3, 3, None), (300, 1.0, 1, None)]


@pytest.mark.parametrize('M,group_frac,T,labels', MATCH_CASES, ids=['M%d-g%s-T%d-%s' % (m, g, t, 'labels' if l else 'all') for m, g, t, l in MATCH_CASES])
def test_match_is_exact(M, group_frac, T, labels):
    C, n_img, n_det = 5, 1 + M % 3, 40 + M % 61
    thresholds = [0.5] if T == 1 else ([0.5, 0.55, 0.75] if T == 3 else list(np.linspace(0.25, 0.95, 15)))
    images = O.dense_case(900 + M + T, n_img, C, M, n_det, group_frac, classes_used=min(2, M), labels=labels)
    ref = O.evaluate(images, C, thresholds, 0.5)
    ev = _evaluator(C, thresholds, 0.5)
    args, kw = _pack(images, n_det + 3, M)
    flags = _u32(ev.add_batch(*args, **kw))
    vscore, vflags = ev._last_virtual[0].cpu().numpy(), _u32(ev._last_virtual[1])
    kept = ev._last_kept.cpu().numpy()
    seen = []
    for i, im in enumerate(images):
        n, m = len(im['det_scores']), len(im['gt_classes'])
        rf = ref['flags'][i].astype(np.int64)
        assert np.array_equal(flags[i, :n], rf), 'image %d: flags differ at %s' % (i, np.nonzero(flags[i, :n] != rf)[0][:8].tolist())
        assert (flags[i, n:] == INVALID).all()
        assert np.array_equal(vflags[i, :m], ref['vflags'][i].astype(np.int64)) and (vflags[i, m:] == INVALID).all(), i
        assert np.array_equal(vscore[i, :m].view(np.uint32), ref['vscore'][i].view(np.uint32)) and (vscore[i, m:] == 0).all(), i
        assert kept[i] == int((rf >> 31 == 0).sum() + (ref['vflags'][i] >> 31 == 0).sum()) and kept[n_img + i] == 0
        seen.append(rf)
    for got, want in ((ev._n_plain, ref['n_plain']), (ev._n_group, ref['n_group']), (ev._gt_imgs, ref['gt_imgs'])):
        assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(ev._correct.cpu().numpy().reshape(len(thresholds), C), ref['correct'])
    live = int((ref['words'] >> 31 == 0).sum())
    assert ev._state.cpu().tolist() == [live, 0, 0, 0]
    seen = np.concatenate(seen)
    valid = seen >> 31 == 0
    assert (valid & (seen & 1 == 1)).any() or group_frac == 1.0               # true positives, unless every box is group-of
    if group_frac > 0:
        assert (valid & ((seen >> 16) & 1 == 1)).any() and any((vf >> 31 == 0).any() for vf in ref['vflags'])
        assert M == 1 or any((vf >> 31 != 0).any() for vf in ref['vflags'])      # and group-of slots without an entry
    else:
        assert all((vf >> 31 != 0).all() for vf in ref['vflags'])
    if labels:
        assert (seen >> 31 == 1).sum() > sum(int((O.match_image({k: v for k, v in im.items() if k != 'labeled_cls'}, C, thresholds)[0] >> 31 == 1).sum())
                                             for im in images)
    # the appended entries, in (image, slot, then virtual (box, threshold)) order
    keep = ref['words'] >> 31 == 0
    assert np.array_equal(ev._bufs[0][:live].cpu().numpy().view(np.uint32), (ref['scores'][keep] + np.float32(0)).view(np.uint32))
    assert np.array_equal(ev._bufs[1][:live].cpu().numpy(), ref['classes'][keep])
    assert np.array_equal(_u32(ev._bufs[2][:live]), ref['words'][keep].astype(np.int64))
    ev.enqueue()
    r = ev.result()
    assert _same(r['ap'], ref['ap']) and r['n'] == live


# ------------------------------------------------------------------------------------------------ sorted AP
def _load(ev, scores, classes, flags, n_plain, n_group):
    """put accumulated entries into the evaluator's device buffers directly (what add_batch calls would have left there)"""
    n = len(scores)
    ev.clear()
    ev._bufs[0][:n] = torch.from_numpy(np.asarray(scores, np.float32)).to(DEV)
    ev._bufs[1][:n] = torch.from_numpy(np.asarray(classes, np.int32)).to(DEV)
    ev._bufs[2][:n] = torch.from_numpy(np.asarray(flags, np.int64).astype(np.uint32).view(np.int32)).to(DEV)
    ev._state[0] = n
    ev._n_plain.copy_(torch.from_numpy(np.asarray(n_plain, np.int32)))
    ev._n_group.copy_(torch.from_numpy(np.asarray(n_group, np.int32)))


def _tile():
    from ood_object_detection_amd import _lib
    return _lib.load().effdet_eval_scale_sort_tile()


def _entries(n, seg, C, T, seed, levels=4096):
    """n entries of which exactly `seg` are valid entries of class 0 (one segment); class 1 has entries but no instances"""
    rs = np.random.RandomState(seed)
    classes = rs.randint(-1, C, n)
    if seg:
        classes[classes == 0] = 2 % C
        classes[rs.permutation(n)[:seg]] = 0
    scores = ((rs.randint(0, levels, n) - levels // 4) / np.float32(levels)).astype(np.float32)
    u = rs.uniform(size=n)
    t = rs.randint(0, T, n)
    all_bits = (1 << T) - 1
    group = (1 << t) | ((all_bits & ~(1 << t)) << 16) | (1 << 15)             # a virtual entry of threshold t
    plain = np.where(u < 0.3, all_bits >> rs.randint(0, T, n), 0) | np.where((u >= 0.3) & (u < 0.4), 1 << (16 + t), 0)
    flags = np.where(u < 0.85, plain, np.where(u < 0.95, group, 1 << 31)).astype(np.int64)
    if seg:
        bad = (classes == 0) & (flags >> 31 == 1)
        flags[bad] = 0
    n_plain = np.array([int(((flags & 1 == 1) & (flags >> 15 & 1 == 0) & (flags >> 31 == 0) & (classes == c)).sum()) + rs.randint(1, 9) for c in range(C)])
    n_group = np.array([int(((flags >> 15 & 1 == 1) & (classes == c)).sum()) + rs.randint(0, 4) for c in range(C)])
    n_plain[1], n_group[1] = 0, 0
    return scores, classes, flags, n_plain, n_group


SIZES = ['2047', '2048', '2049', 'tile-1', 'tile', 'tile+1']


@pytest.mark.parametrize('which', SIZES)
@pytest.mark.parametrize('w', [0.5, 0.3])
def test_sorted_order_ap_and_pooled_ap_are_bitwise(which, w):
    """one-class segments of 2047 / 2048 / 2049 entries around the AP chunk (the other classes hold about as many again), and
    tile - 1 / tile / tile + 1 entries in all around the sort tile"""
    tile = _tile()
    C, T = 3, 3
    if 'tile' in which:
        n = eval(which, {'tile': tile})
        seg = 0
    else:
        seg = int(which)
        n = 2 * seg + 100
    scores, classes, flags, n_plain, n_group = _entries(n, seg, C, T, 2000 + n % 997)
    ev = _evaluator(C, (0.5, 0.55, 0.75), w, use_weighted_mean_ap=True, capacity=max(n, 2 * tile + 5))
    _load(ev, scores, classes, flags, n_plain, n_group)
    ev.enqueue()
    r = ev.result()
    ref = O.ap_from_entries(scores, classes, flags, n_plain, n_group, w, C, T)
    cls, sc, fl = ev.sorted()
    rc, rs_, rf = ref['sorted']
    if seg:
        assert int((rc == 0).sum()) == seg
    assert np.array_equal(cls, rc) and np.array_equal(sc.view(np.uint32), rs_.view(np.uint32)) and np.array_equal(fl, rf)
    psc, pfl = ev.sorted_pooled()
    assert np.array_equal(psc.view(np.uint32), ref['pooled'][1].view(np.uint32)) and np.array_equal(pfl, ref['pooled'][2])
    assert (ref['pooled'][0] != 1).all() and (rc == 1).any()                  # class 1 has entries and no instances: left out
    assert r['n'] == n and r['lost'] == 0
    assert np.array_equal(r['n_plain'], n_plain) and np.array_equal(r['n_group'], n_group)
    assert np.isnan(r['ap'][:, 1]).all() and np.isfinite(r['ap'][:, [0, 2]]).all() and (r['ap'][:, [0, 2]] > 0).all()
    print('AP', r['ap'].tolist(), 'pooled', r['weighted_ap'].tolist())
    assert _same(r['ap'], ref['ap']), (r['ap'], ref['ap'])
    assert _same(r['weighted_ap'], ref['pooled_ap']), (r['weighted_ap'], ref['pooled_ap'])


def test_pooled_ties_stand_in_class_then_arrival_order():
    """few distinct scores, so equal scores cross classes: the pooled order is (class, arrival) inside a tie"""
    C, T, n = 4, 1, 3000
    scores, classes, flags, n_plain, n_group = _entries(n, 0, C, T, 77, levels=8)
    ev = _evaluator(C, (0.5,), 1.0, use_weighted_mean_ap=True, capacity=n + 7)
    _load(ev, scores, classes, flags, n_plain, n_group)
    ev.enqueue()
    r = ev.result()
    ref = O.ap_from_entries(scores, classes, flags, n_plain, n_group, 1.0, C, T)
    psc, pfl = ev.sorted_pooled()
    assert len(np.unique(psc)) <= 8 and np.array_equal(pfl, ref['pooled'][2]) and np.array_equal(psc, ref['pooled'][1])
    assert _same(r['weighted_ap'], ref['pooled_ap']) and _same(r['ap'], ref['ap'])
    # the check has teeth: with the ties in arrival order alone the pooled AP is another
    ok = np.nonzero((flags >> 31 == 0) & (classes >= 0) & (classes != 1))[0]
    ok = ok[np.argsort(-scores[ok], kind='stable')]
    total = float(n_plain.sum() + 1.0 * n_group.sum())
    assert abs(O.ap_segment(flags[ok], 0, 1.0, total) - ref['pooled_ap'][0]) > 1e-9


# ------------------------------------------------------------------------------------------------ against the PASCAL evaluator
@pytest.mark.parametrize('w', [0.0, 1.0])
def test_without_group_of_flags_the_ap_block_equals_the_dataset_evaluator(w):
    from ood_object_detection_amd.effdet.evaluation import DatasetDetectionEvaluator
    g = _golden()
    images, C = O.fixture_case(g, 'a', difficult=True)
    thresholds = (0.5, 0.55, 0.75)
    old = DatasetDetectionEvaluator(_cats(C), iou_thresholds=thresholds, capacity=4096, device=DEV)
    new = _evaluator(C, thresholds, w, capacity=4096)
    args, kw = _pack(images, 22, 5)
    f_old = old.add_batch(*args, kw['gt_difficult'])
    f_new = new.add_batch(*args, gt_difficult=kw['gt_difficult'])             # no group-of table at all
    assert np.array_equal(f_old.cpu().numpy(), f_new.cpu().numpy())
    old.enqueue(), new.enqueue()
    a, b = old.result(), new.result()
    assert _same(a['ap'], b['ap']) and np.isfinite(a['ap']).any()
    T = len(thresholds)
    assert np.array_equal(a['block'][8:8 + T * C], b['block'][8:8 + T * C]) and a['n'] == b['n']
    assert np.array_equal(a['gt_count'], b['n_plain']) and np.array_equal(a['gt_imgs'], b['gt_imgs']) and np.array_equal(a['correct'], b['correct'])
    assert (b['n_group'] == 0).all()
    zero = new.add_batch(*args, gt_difficult=kw['gt_difficult'], gt_group_of=torch.zeros_like(kw['gt_group_of']))
    assert np.array_equal(zero.cpu().numpy(), f_new.cpu().numpy())           # a table of zeros is no table


def test_device_equals_the_reference_fixture():
    """the device's own order of the sum against the reference's: 1e-12, as for evaluation_scale.npz"""
    from ood_object_detection_amd.effdet.evaluation import OpenImagesChallengeEvaluator, WeightedPascalDetectionEvaluator
    g = _golden()
    thresholds = tuple(float(t) for t in g['thresholds'])
    for tag in ('a', 'b'):
        images, C = O.fixture_case(g, tag)
        for k, w in enumerate(g['weights']):
            ev = _evaluator(C, thresholds, float(w), capacity=4096)
            args, kw = _pack(images, 26, 5)
            ev.add_batch(*args, gt_group_of=kw['gt_group_of'])
            ev.enqueue()
            assert np.allclose(ev.result()['ap'], g[tag + '_oi_ap'][k], rtol=0, atol=1e-12, equal_nan=True), (tag, w)
        images, C = O.fixture_case(g, tag, labels=True)
        ev = OpenImagesChallengeEvaluator(_cats(C), iou_thresholds=thresholds, capacity=4096, device=DEV)
        args, kw = _pack(images, 26, 5)
        ev.add_batch(*args, gt_group_of=kw['gt_group_of'], labeled_cls=kw['labeled_cls'])
        m = ev.evaluate()
        assert np.allclose(ev.result()['ap'], g[tag + '_ch_ap'], rtol=0, atol=1e-12, equal_nan=True)
        assert abs(m['OpenImagesDetectionChallenge_Precision/mAP@0.5IOU'] - g[tag + '_ch_map'][0]) <= 1e-12
        images, C = O.fixture_case(g, tag, difficult=True)
        ev = WeightedPascalDetectionEvaluator(_cats(C), iou_thresholds=thresholds, capacity=4096, device=DEV)
        args, kw = _pack(images, 26, 5)
        ev.add_batch(*args, gt_difficult=kw['gt_difficult'])
        m = ev.evaluate()
        r = ev.result()
        assert np.allclose(r['ap'], g[tag + '_wp_ap'], rtol=0, atol=1e-12, equal_nan=True)
        assert np.allclose(r['weighted_ap'], g[tag + '_wp_map'], rtol=0, atol=1e-12)
        assert list(m)[0] == 'WeightedPascalBoxes_Precision/mAP@0.5IOU' and abs(list(m.values())[0] - g[tag + '_wp_map'][0]) <= 1e-12
        assert m['AP@0.75IOU/c0'] == r['ap'][2, 0] or np.isnan(r['ap'][2, 0])


# ------------------------------------------------------------------------------------------------ mechanics
def _mechanics_case():
    C, M, n_det = 4, 40, 50
    return O.dense_case(31, 7, C, M, n_det, 0.4, labels=2), C, M, n_det, (0.5, 0.55, 0.75)


def _run_split(ev, images, parts, max_det, M):
    ev.clear()
    for idx in np.array_split(np.arange(len(images)), parts):
        args, kw = _pack([images[i] for i in idx], max_det, M, K=2)
        ev.add_batch(*args, **kw)
    ev.enqueue()
    return ev.result()['block']


def test_result_block_is_bit_identical_across_splits():
    images, C, M, n_det, thresholds = _mechanics_case()
    ev = _evaluator(C, thresholds, 0.3, use_weighted_mean_ap=True, capacity=4096)
    blocks = [_run_split(ev, images, parts, n_det, M) for parts in (1, 2, 5, 1)]
    for b in blocks[1:]:
        assert np.array_equal(b, blocks[0])
    ref = O.evaluate(images, C, thresholds, 0.3)
    r = ev.result()
    assert _same(r['ap'], ref['ap']) and _same(r['weighted_ap'], ref['pooled_ap'])
    assert r['n'] == int((ref['words'] >> 31 == 0).sum()) and any((vf >> 31 == 0).any() for vf in ref['vflags'])


def test_add_batch_and_enqueue_in_a_captured_graph():
    images, C, M, n_det, thresholds = _mechanics_case()
    ev = _evaluator(C, thresholds, 0.5, use_weighted_mean_ap=True, capacity=4096)
    (a1, k1), (a2, k2) = _pack(images[:3], n_det, M, K=2), _pack(images[3:], n_det, M, K=2)
    ev.add_batch(*a1, **k1)
    ev.add_batch(*a2, **k2)
    ev.enqueue()
    eager = ev.result()['block']
    ev.clear()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ev.add_batch(*a1, **k1)
        ev.add_batch(*a2, **k2)
        ev.enqueue()
    ev.clear()
    ev._result.zero_()
    graph.replay()
    assert np.array_equal(ev.result()['block'], eager)


def test_an_overflow_by_virtual_entries_alone_is_lost_and_reported():
    images, C, M, n_det, thresholds = _mechanics_case()
    ref = O.evaluate(images, C, thresholds, 1.0)
    dets = int(sum((f >> 31 == 0).sum() for f in ref['flags']))
    virtual = int(sum((vf >> 31 == 0).sum() for vf in ref['vflags']))
    assert virtual >= 3
    ev = _evaluator(C, thresholds, 1.0, capacity=dets + virtual - 2)          # every detection fits, two virtual entries do not
    args, kw = _pack(images, n_det, M, K=2)
    ev.add_batch(*args, **kw)
    assert ev._state.cpu().tolist()[:2] == [dets + virtual - 2, 2]
    ev.enqueue()
    with pytest.raises(RuntimeError, match=r'\b2 entries were lost\b'):
        ev.result()
    none = _evaluator(C, thresholds, 0.0, capacity=dets)                      # weight 0 emits nothing: the same capacity suffices
    none.add_batch(*args, **kw)
    none.enqueue()
    assert none.result()['n'] == dets


def test_argument_checks_on_the_device():
    ev = _evaluator(3, (0.5,), 1.0, capacity=64)
    det, cnt = torch.zeros(2, 4, 6, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
    gtb, gtc = torch.zeros(2, 3, 4, device=DEV), torch.zeros(2, 3, dtype=torch.int64, device=DEV)
    for kw in (dict(gt_group_of=torch.zeros(2, 2, dtype=torch.bool)), dict(gt_difficult=torch.zeros(3, 3, dtype=torch.bool)),
               dict(labeled_cls=torch.zeros(3, 1, dtype=torch.int64)), dict(labeled_cls=torch.zeros(2, dtype=torch.int64))):
        with pytest.raises(ValueError):
            ev.add_batch(det, cnt, gtb, gtc, **kw)
    with pytest.raises(ValueError):
        ev.add_batch(det[:, :, :5], cnt, gtb, gtc)
    with pytest.raises(ValueError):
        ev.add_batch(det, cnt[:1], gtb, gtc)
    ev.add_batch(det, cnt, gtb, gtc, labeled_cls=torch.zeros(2, 0, dtype=torch.int64))      # the empty list is a list
    assert ev._state.cpu().tolist() == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ end to end
class _Parser:
    def __init__(self, images, C, labels=False):
        self.img_ids = list(range(len(images)))
        self.cat_ids = list(range(1, C + 1))
        self.cat_dicts = _cats(C)
        self._images, self._labels = images, labels

    def get_ann_info(self, i):
        im = self._images[i]
        out = dict(bbox=im['gt_boxes'], cls=im['gt_classes'] + 1, group_of=im['gt_group_of'])
        if self._labels:
            out['img_cls'] = im['labeled_cls'] + 1
        return out


class _Dataset:
    def __init__(self, parser):
        self.parser = parser


def _predictions(images, max_det):
    return torch.from_numpy(O.pack(images, max_det, len(images[0]['gt_classes']))[0]).to(DEV)     # rows of zeros (class 0) are padding


def test_open_images_evaluator_end_to_end_with_group_of_boxes():
    from ood_object_detection_amd.effdet import evaluator as E
    C, M, n_det = 4, 12, 30
    images = O.dense_case(41, 5, C, M, n_det, 0.4, labels=2)
    for im in images:
        im['gt_difficult'][:] = False
        keep = im['det_scores'] > 0                                           # rows of zeros are padding for add_predictions
        for k in ('det_boxes', 'det_scores', 'det_classes'):
            im[k] = im[k][keep]
    det = _predictions(images, n_det)
    plain = [{k: v for k, v in im.items() if k != 'labeled_cls'} for im in images]
    for name, w, ims, prefix in (('openimages-v5', 0.0, plain, 'OpenImagesV2'), ('openimages-v5', 0.5, plain, 'OpenImagesV2'),
                                 ('openimages_challenge', 1.0, images, 'OpenImagesDetectionChallenge')):
        kw = dict(group_of_weight=w) if 'challenge' not in name else {}
        ev = E.create_evaluator(name, _Dataset(_Parser(images, C, labels='challenge' in name)), capacity=4096, **kw)
        order = [3, 0, 4]
        ev.add_predictions(det[order], dict(img_idx=torch.tensor(order)))
        ev.add_predictions(det[[1, 2]], dict(img_idx=torch.tensor([1, 2])))
        metric = ev.evaluate()
        ref = O.evaluate([ims[i] for i in order + [1, 2]], C, (0.5,), w)
        assert any((vf >> 31 == 0).any() for vf in ref['vflags']) == (w > 0) and any(((f >> 16) & 1).any() for f in ref['flags'])
        assert metric == float(np.nanmean(ref['ap'][0])) and 0 < metric < 1
        assert ev.metrics[prefix + '_Precision/mAP@0.5IOU'] == metric
        for c in range(C):
            assert _same(np.array(ev.metrics['AP@0.5IOU/c%d' % c]), np.array(ref['ap'][0, c]))


def test_single_image_api_takes_group_of_and_verified_labels():
    from ood_object_detection_amd.effdet.evaluation import OpenImagesChallengeEvaluator
    C, M, n_det = 4, 12, 30
    images = O.dense_case(43, 4, C, M, n_det, 0.4, labels=1)
    for im in images:
        im['gt_difficult'][:] = False
    ev = OpenImagesChallengeEvaluator(_cats(C), iou_thresholds=(0.5, 0.75), evaluate_corlocs=True, capacity=4096, device=DEV)
    for i, im in enumerate(images):
        ev.add_single_ground_truth_image_info(i, {'bbox': im['gt_boxes'], 'cls': im['gt_classes'] + 1, 'group_of': im['gt_group_of'],
                                                  'labeled_cls' if i % 2 else 'img_cls': im['labeled_cls'] + 1})
    for i, im in enumerate(images[:-1]):                                      # the last image's ground truth counts without detections
        ev.add_single_detected_image_info(i, {'bbox': im['det_boxes'], 'scores': im['det_scores'], 'cls': im['det_classes'] + 1})
    m = ev.evaluate()
    last = dict(images[-1], det_boxes=np.zeros((0, 4), np.float32), det_scores=np.zeros(0, np.float32), det_classes=np.zeros(0, np.int64))
    ref = O.evaluate(images[:-1] + [last], C, (0.5, 0.75), 1.0)
    r = ev.result()
    assert _same(r['ap'], ref['ap']) and np.array_equal(r['n_group'], ref['n_group']) and np.array_equal(r['correct'], ref['correct'])
    assert m['OpenImagesDetectionChallenge_Precision/mAP@0.75IOU'] == float(np.nanmean(ref['ap'][1]))
    assert 'CorLoc@0.5IOU/c0' in m and 'OpenImagesDetectionChallenge_Precision/meanCorLoc@0.5IOU' in m
    assert sum(int((f >> 31 == 1).sum()) for f in ref['flags']) > 0
