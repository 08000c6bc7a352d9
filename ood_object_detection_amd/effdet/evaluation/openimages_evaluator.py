"""OpenImages detection evaluation on the device (csrc/openimages_eval.hip): the reference's `OpenImagesDetectionEvaluator`,
`OpenImagesChallengeEvaluator` and `WeightedPascalDetectionEvaluator` (effdet/evaluation/detection_evaluator.py:329-347, 368-589)
on `DatasetDetectionEvaluator`'s storage, `enqueue`, `result` and `clear`, at up to 15 IoU thresholds from one matching pass.

Group-of boxes (per_image_evaluation.py:305-473): a detection first looks at the boxes of its class that are not group-of, as in
the PASCAL protocol; one that is neither a true positive nor ignored there is absorbed by the group-of box of its class that covers
most of it (intersection over the detection's area >= the threshold) and leaves the entries.  With `group_of_weight` w > 0 every
group-of box that absorbed a detection with a score > 0 counts as ONE true positive of weight w at the largest absorbed score, and
every group-of box as w instances; with w = 0 the absorbed detections just leave.  `use_weighted_mean_ap`: the mAP metric is the AP
over the pooled entries of all classes with instances (object_detection_evaluation.py:221-264).  The Challenge variant drops, per
image, the detections of classes that are neither a box's class nor a verified image-level label.

A box flagged both difficult and group-of is ill-defined in the reference (its AP can raise): here it absorbs detections like any
group-of box and counts neither as an instance nor as group weight.  Not built: masks, precision / recall curves, recall bounds,
label-hierarchy expansion.  No CPU fallback.
"""
import ctypes

import numpy as np
import torch

from ... import _lib
from .dataset_evaluator import RESULT_HEAD, DatasetDetectionEvaluator
from .detection_evaluator import create_category_index

MAX_THRESHOLDS = 15                  # bit 15 of a flag word marks a group-of box's entry


def parse_openimages_result(block, T, C):
    """the host copy of a result block -> dict(n, lost, nan_scores, ap [T, C] float64, weighted_ap [T] float64 (NaN unless asked
    for), n_plain [C], n_group [C], gt_imgs [C], correct [T, C])"""
    w = block.numpy() if torch.is_tensor(block) else np.asarray(block)
    assert int(w[3]) == T and int(w[4]) == C
    o = RESULT_HEAD
    ap = w[o:o + T * C].view(np.float64).reshape(T, C).copy()
    o += T * C
    pooled = w[o:o + T].view(np.float64).copy()
    o += T
    return dict(n=int(w[0]), lost=int(w[1]), nan_scores=int(w[2]), ap=ap, weighted_ap=pooled, n_plain=w[o:o + C].copy(),
                n_group=w[o + C:o + 2 * C].copy(), gt_imgs=w[o + 2 * C:o + 3 * C].copy(),
                correct=w[o + 3 * C:o + 3 * C + T * C].reshape(T, C).copy())


class OpenImagesDetectionEvaluator(DatasetDetectionEvaluator):
    """categories, capacity, device, storage: as DatasetDetectionEvaluator; the capacity also holds the group-of boxes' entries (at
    most one per box and threshold).  iou_thresholds: 1 to 15, ascending.  group_of_weight: finite, >= 0."""

    def __init__(self, categories, iou_thresholds=(0.5,), group_of_weight=0.0, use_weighted_mean_ap=False, evaluate_corlocs=False,
                 metric_prefix='OpenImagesV5', capacity=1 << 20, device='cuda:0', storage=None):
        thr = list(iou_thresholds)
        if not 1 <= len(thr) <= MAX_THRESHOLDS:
            raise ValueError('1 to %d IoU thresholds, got %d' % (MAX_THRESHOLDS, len(thr)))
        self._weight = float(group_of_weight)
        if not 0.0 <= self._weight < float('inf'):
            raise ValueError('group_of_weight must be finite and not negative, got %r' % (group_of_weight,))
        self._pooled = bool(use_weighted_mean_ap)
        super().__init__(categories, iou_thresholds=thr, capacity=capacity, evaluate_corlocs=evaluate_corlocs,
                         metric_prefix=metric_prefix, device=device, storage=storage)
        T, C = len(self._thresholds), self._num_classes
        self._counters = torch.zeros(3 * C + T * C, dtype=torch.int32, device=self.device)
        self._n_plain, self._n_group = self._counters[:C], self._counters[C:2 * C]
        self._gt_imgs, self._correct = self._counters[2 * C:3 * C], self._counters[3 * C:]
        self._gt_count = self._n_plain
        self._metric_names = [self._metric_prefix + 'Precision/mAP@{}IOU'.format(self._thresholds[0])]
        if evaluate_corlocs:
            self._metric_names.append(self._metric_prefix + 'Precision/meanCorLoc@{}IOU'.format(self._thresholds[0]))
        self._last_virtual = None

    def _alloc_blocks(self, T, C, dev):
        nb = self.lib.effdet_openimages_sorted_workspace_bytes(self.capacity, C, int(self._pooled))
        self._ws = torch.empty(nb // 8, dtype=torch.int64, device=dev)
        self._result = torch.zeros(self.lib.effdet_openimages_sorted_result_bytes(T, C) // 8, dtype=torch.int64, device=dev)

    def _accepts_group_of(self):
        return True

    def _default_labels(self):
        """the label list of an image that came without one (None: every class is evaluatable)"""
        return None

    # ---- native entry -------------------------------------------------------------------------------------------------------------
    def add_batch(self, det, count, gt_boxes, gt_cls, gt_group_of=None, gt_difficult=None, labeled_cls=None):
        """det [B, max_det, 6] rows x1,y1,x2,y2,score,class (1-based) in descending score order, `count[b]` valid rows; gt_boxes
        [B, M, 4] yxyx, gt_cls [B, M] 1-based (<= 0: padding), gt_group_of / gt_difficult [B, M] bool or None; labeled_cls [B, K]
        int64 1-based verified image-level labels (<= 0: padding) or None: with a list, detections of classes that are neither a
        box's class nor in the list are dropped.  -> flag words [B, max_det] int32: bit t = true positive at threshold t, bit
        16 + t = ignored or absorbed by a group-of box there, bit 31 (negative) = dropped.  `self._last_virtual`: (vscore, vflags)
        [B, M, T], the group-of boxes' entries of this batch."""
        dev = self.device
        det = det.to(device=dev, dtype=torch.float32).contiguous()
        count = count.to(device=dev, dtype=torch.int32).contiguous()
        gt_boxes = gt_boxes.to(device=dev, dtype=torch.float32).contiguous()
        gt_cls = gt_cls.to(device=dev, dtype=torch.int64).contiguous()
        if det.dim() != 3 or det.shape[2] != 6 or gt_boxes.dim() != 3 or gt_boxes.shape[2] != 4:
            raise ValueError('det must be [B, max_det, 6] and gt_boxes [B, M, 4]')
        B, max_det, _ = det.shape
        M = gt_boxes.shape[1]
        if gt_boxes.shape[0] != B or tuple(gt_cls.shape) != (B, M) or count.numel() != B:
            raise ValueError('count [B], gt_boxes [B, M, 4] and gt_cls [B, M] must agree with det')
        tables = []
        for name, t in (('gt_group_of', gt_group_of), ('gt_difficult', gt_difficult)):
            if t is not None:
                t = torch.as_tensor(t).to(device=dev, dtype=torch.uint8).contiguous()
                if tuple(t.shape) != (B, M):
                    raise ValueError('%s must be [B, M]' % name)
            tables.append(t)
        if labeled_cls is None:
            labeled_cls = self._default_labels()
            if labeled_cls is not None:
                labeled_cls = labeled_cls.expand(B, -1)
        if labeled_cls is not None:
            labeled_cls = labeled_cls.to(device=dev, dtype=torch.int64).contiguous()
            if labeled_cls.dim() != 2 or labeled_cls.shape[0] != B:
                raise ValueError('labeled_cls must be [B, K]')
            if labeled_cls.shape[1] == 0:                                     # the empty list: its pointer is not null
                labeled_cls = torch.zeros(B, 1, dtype=torch.int64, device=dev)
        if M == 0:
            gt_boxes = torch.zeros(B, 1, 4, dtype=torch.float32, device=dev)
            gt_cls = torch.zeros(B, 1, dtype=torch.int64, device=dev)
            tables, M = [None, None], 1
        T = len(self._thresholds)
        if self.lib.effdet_openimages_match_lds_bytes(M, self._num_classes, T) > 64 * 1024:
            raise ValueError('%d ground-truth boxes an image at %d thresholds and %d classes exceed 64 KiB of LDS' % (M, T, self._num_classes))
        flags = torch.empty(B, max_det, dtype=torch.int32, device=dev)
        vscore = torch.empty(B, M, T, dtype=torch.float32, device=dev)
        vflags = torch.empty(B, M, T, dtype=torch.int32, device=dev)
        kept = torch.empty(2 * B, dtype=torch.int32, device=dev)
        st = self._st()
        ptr = lambda t: t.data_ptr() if t is not None else None
        _lib.check(self.lib.effdet_openimages_match(st, det.data_ptr(), count.data_ptr(), gt_boxes.data_ptr(), gt_cls.data_ptr(),
                                                    ptr(tables[1]), ptr(tables[0]), ptr(labeled_cls),
                                                    labeled_cls.shape[1] if labeled_cls is not None else 0, B, max_det, M,
                                                    self._num_classes, self._thr, T, int(self._weight > 0), flags.data_ptr(),
                                                    vscore.data_ptr(), vflags.data_ptr(), kept.data_ptr(), self._n_plain.data_ptr(),
                                                    self._n_group.data_ptr(), self._gt_imgs.data_ptr(), self._correct.data_ptr()),
                   'effdet_openimages_match')
        _lib.check(self.lib.effdet_openimages_append(st, det.data_ptr(), flags.data_ptr(), gt_cls.data_ptr(), vscore.data_ptr(),
                                                     vflags.data_ptr(), kept.data_ptr(), B, max_det, M, T, self._bufs[0].data_ptr(),
                                                     self._bufs[1].data_ptr(), self._bufs[2].data_ptr(), self.capacity,
                                                     self._state.data_ptr()), 'effdet_openimages_append')
        self._last_virtual, self._last_kept = (vscore, vflags), kept
        return flags

    def enqueue(self):
        """Sort + metrics into the result block on the device; no host synchronisation."""
        self._flush_pending()
        _lib.check(self.lib.effdet_openimages_sorted(self._st(), self._bufs[0].data_ptr(), self._bufs[1].data_ptr(),
                                                     self._bufs[2].data_ptr(), self.capacity, -1, self._state.data_ptr(),
                                                     len(self._thresholds), self._num_classes, ctypes.c_double(self._weight),
                                                     int(self._pooled), self._n_plain.data_ptr(), self._n_group.data_ptr(),
                                                     self._gt_imgs.data_ptr(), self._correct.data_ptr(), self._ws.data_ptr(),
                                                     self._ws.numel() * 8, self._result.data_ptr()), 'effdet_openimages_sorted')

    def result(self):
        """The result block of the last `enqueue()` (ONE device-to-host copy) -> dict(n, lost, nan_scores, ap [T, C], weighted_ap
        [T], n_plain, n_group, gt_imgs, correct [T, C], gt_count = n_plain, block: the raw int64 words)."""
        block = self._result.cpu()
        r = parse_openimages_result(block, len(self._thresholds), self._num_classes)
        if r['lost']:
            raise RuntimeError('%d entries were lost: more detections and group-of entries were added than the capacity of %d holds'
                               % (r['lost'], self.capacity))
        r['gt_count'] = r['n_plain']
        r['block'] = block.numpy()
        return r

    def _sorted_offsets(self):
        return [self.lib.effdet_openimages_sorted_offset(self.capacity, self._num_classes, w) for w in (0, 1)]

    def sorted_pooled(self):
        """After `enqueue()` with use_weighted_mean_ap: (score [k] float32, flag word [k] uint32) of the pooled entries in their
        order (debug / test accessor; synchronises)."""
        if not self._pooled:
            raise RuntimeError('constructed without use_weighted_mean_ap=True')
        ws = self._ws.view(torch.uint8)
        ko, vo = [self.lib.effdet_openimages_sorted_offset(self.capacity, self._num_classes, w) for w in (2, 3)]
        n = min(int(self._state[0].item()), self.capacity)
        keys = ws[ko:ko + 8 * n].cpu().numpy().view(np.uint64)
        words = ws[vo:vo + 4 * n].cpu().numpy().view(np.uint32)
        k = ~(keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        bits = np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k)
        valid = (keys >> np.uint64(32)) == 0
        return bits.view(np.float32)[valid], words[valid]

    # ---- reference API --------------------------------------------------------------------------------------------------------------
    def _gt_flags(self, gt_dict, n):
        """(difficult, group_of, labels) of one image's ground-truth dict: [n] bool tensors or None, [K] int64 1-based or None"""
        out = []
        for k in ('difficult', 'group_of'):
            t = None
            if k in gt_dict and (np.asarray(gt_dict[k]).size or not n):       # an empty array beside boxes counts as absent
                t = torch.as_tensor(np.asarray(gt_dict[k]).astype(bool)).reshape(-1)
                if t.numel() != n:
                    raise ValueError('%s: one flag per ground-truth box' % k)
            out.append(t)
        labels = None
        for k in ('img_cls', 'labeled_cls'):                                  # detection_evaluator.py:538-541
            if k in gt_dict:
                labels = torch.as_tensor(np.asarray(gt_dict[k]), dtype=torch.int64).reshape(-1)
                break
        return out[0], out[1], labels

    def _add_image(self, det, count, gt_b, gt_c, gt_d):
        difficult, group_of, labels = gt_d if gt_d is not None else (None, None, None)
        if labels is None and self._default_labels() is not None:
            labels = self._default_labels()[0]
        one = lambda t: t[None] if t is not None else None
        self.add_batch(det, count, gt_b[None], gt_c[None], gt_group_of=one(group_of), gt_difficult=one(difficult),
                       labeled_cls=one(labels))

    def evaluate(self, task_categories=None, batch_cats=None):
        """Metric dict with the reference's keys (detection_evaluator.py:268-305) at every threshold; with use_weighted_mean_ap
        'Precision/mAP' is the pooled AP.  With more than one threshold 'Precision/mAP@[first:last]IOU' = the mean of the
        per-threshold figures that are not NaN."""
        self.enqueue()
        r = self.result()
        ap = r['ap']
        with np.errstate(invalid='ignore', divide='ignore'):
            corloc = np.where(r['gt_imgs'][None] == 0, np.nan, r['correct'].astype(float) / r['gt_imgs'][None])
        if task_categories is None:
            index = create_category_index(self._categories)
            task_categories = [index[i + 1]['name'] for i in range(self._num_classes)]
        nanmean = lambda v: float(np.nanmean(v)) if np.isfinite(v).any() else float('nan')
        out, maps = {}, []
        for t, thr in enumerate(self._thresholds):
            maps.append(float(r['weighted_ap'][t]) if self._pooled else nanmean(ap[t]))
            out[self._metric_prefix + 'Precision/mAP@{}IOU'.format(thr)] = maps[-1]
            if self._evaluate_corlocs:
                out[self._metric_prefix + 'Precision/meanCorLoc@{}IOU'.format(thr)] = nanmean(corloc[t])
            for idx, category_name in enumerate(task_categories):
                if batch_cats is not None and idx not in batch_cats:
                    continue
                out['AP@{}IOU/{}'.format(thr, category_name)] = ap[t, idx]
                if self._evaluate_corlocs:
                    out['CorLoc@{}IOU/{}'.format(thr, category_name)] = corloc[t, idx]
        if len(self._thresholds) > 1:
            out[self._metric_prefix + 'Precision/mAP@[{}:{}]IOU'.format(self._thresholds[0], self._thresholds[-1])] = nanmean(np.array(maps))
        return out


class OpenImagesChallengeEvaluator(OpenImagesDetectionEvaluator):
    """effdet/evaluation/detection_evaluator.py:453-589, box mode: group-of boxes weigh 1 by default, and per image only the classes of
    its boxes and its verified image-level labels (`img_cls`, else `labeled_cls`; `labeled_cls` of `add_batch`) are evaluated.  An
    image without a list has the empty list: only its boxes' classes count."""

    def __init__(self, categories, iou_thresholds=(0.5,), evaluate_corlocs=False, group_of_weight=1.0, **kw):
        kw.setdefault('metric_prefix', 'OpenImagesDetectionChallenge')
        super().__init__(categories, iou_thresholds=iou_thresholds, group_of_weight=group_of_weight,
                         evaluate_corlocs=evaluate_corlocs, **kw)

    def _default_labels(self):
        return torch.zeros(1, 1, dtype=torch.int64)


class WeightedPascalDetectionEvaluator(OpenImagesDetectionEvaluator):
    """effdet/evaluation/detection_evaluator.py:329-347: the PASCAL protocol whose first metric is the AP over the pooled entries of all
    classes."""

    def __init__(self, categories, iou_thresholds=(0.5,), **kw):
        kw.setdefault('metric_prefix', 'WeightedPascalBoxes')
        super().__init__(categories, iou_thresholds=iou_thresholds, group_of_weight=0.0, use_weighted_mean_ap=True,
                         evaluate_corlocs=False, **kw)
