"""Open-set detection evaluation on the device (csrc/eval_scale.hip): the evaluation of `DatasetDetectionEvaluator` with one more
class, the unknown class `U = C + 1`, in the ground truth (`gt_cls == U`) and in the detections (`det[..., 5] == U`, e.g. from
`ood.relabel_unknown`), and the three open-set metrics on top of it:

  U-Recall  recall of the unknown class (with U-Precision and U-AP: the unknown class is matched like any other);
  A-OSE     absolute open-set error (Miller et al. 2018): the known-class detections whose IoU with an unknown ground-truth box
            reaches the threshold, true positives of their own class or not (as OWOD counts them);
  WI        wilderness impact (Dhamija et al. 2020) as OWOD (Joseph et al. 2021) computes it: per known class the position of
            the sorted list at which recall is nearest `recall_level` (`min(range(len(rec)), key=lambda i: abs(rec[i] - level))`),
            WI = (open detections up to these positions) / (detections not ignored up to them), summed over the known classes
            that have ground truth and a detection.

`add_batch` = matching + one launch for the open words + one append of both words; `enqueue` = the same sort with a second
payload word, the same AP kernel, one more launch for the counts; `result()` is the one device-to-host copy.  Capturable,
bit-identical across runs and splits, no CPU fallback.
"""
import numpy as np
import torch

from ... import _lib
from .dataset_evaluator import RESULT_HEAD, DatasetDetectionEvaluator, parse_result
from .detection_evaluator import create_category_index

OPEN_MATRICES = ('n_det', 'tp', 'open_total', 'k_star', 'pos', 'rank_at', 'open_at')


def _check_level(recall_level):
    level = float(recall_level)
    if not (0.0 < level <= 1.0):
        raise ValueError('recall_level must lie in (0, 1], got %r' % (recall_level,))
    return level


def k_star_closed_form(level, n_gt, tp, first_is_tp):
    """The cumulative true-positive count whose recall k / n_gt is nearest `level` in float64 among the reachable counts
    k_min .. tp (k_min = 1 when position 0 is a true positive), ties to the smaller count: what the kernel computes."""
    k_min, best, k_star = (1 if first_is_tp else 0), None, 0
    base = int(np.floor(np.float64(level) * np.float64(n_gt)))
    for d in (-1, 0, 1, 2):
        k = min(max(base + d, k_min), tp)
        dist = abs(np.float64(k) / np.float64(n_gt) - np.float64(level))
        if best is None or dist < best:
            best, k_star = dist, k
    return k_star


def parse_open_result(block, T, num_classes):
    """the host copy of a result block of effdet_eval_open_sorted -> the dict of `parse_result` over num_classes = C + 1 classes
    plus the seven int64 matrices [T, C + 1] of OPEN_MATRICES"""
    w = block.numpy() if torch.is_tensor(block) else np.asarray(block)
    base = RESULT_HEAD + 2 * T * num_classes + 2 * num_classes
    r = parse_result(w[:base], T, num_classes)
    for k, name in enumerate(OPEN_MATRICES):
        r[name] = w[base + k * T * num_classes:base + (k + 1) * T * num_classes].reshape(T, num_classes).copy()
    r['tp_at'] = r['k_star'].copy()
    return r


def open_set_metrics(r, num_known):
    """float64 metrics from the integers of `parse_open_result`: recall, precision, precision_at_recall [T, C + 1]; u_recall,
    u_precision, u_ap, a_ose, wi [T]"""
    C = num_known
    gt = r['gt_count'].astype(np.float64)[None]
    with np.errstate(invalid='ignore', divide='ignore'):
        out = dict(recall=r['tp'] / gt, precision=r['tp'] / r['n_det'].astype(np.float64),
                   precision_at_recall=r['tp_at'] / r['rank_at'].astype(np.float64))
        in_s = (r['gt_count'][None, :C] > 0) & (r['pos'][:, :C] >= 0)
        num = np.where(in_s, r['open_at'][:, :C], 0).sum(1)
        den = np.where(in_s, r['rank_at'][:, :C], 0).sum(1)
        out['wi'] = np.where(den > 0, num / np.where(den > 0, den, 1).astype(np.float64), np.nan)
    out['a_ose'] = r['open_total'][:, :C].sum(1)
    out['u_recall'], out['u_precision'], out['u_ap'] = out['recall'][:, C], out['precision'][:, C], r['ap'][:, C]
    return out


class OpenSetDetectionEvaluator(DatasetDetectionEvaluator):
    """categories: the KNOWN classes [{'id': 1..C, 'name': ...}]; the unknown class is `C + 1` and is not listed (a category named
    'unknown' raises; the unknown class listed under any other name cannot be told from a known one and would make C + 2
    classes).  recall_level: the recall at which WI is taken.  evaluate_corlocs, metric_prefix: as `DatasetDetectionEvaluator`, over
    the known classes.  storage: optional caller-owned (scores float32, classes int32, flags int32, open int32) 1-d GPU tensors of
    at least `capacity` entries."""

    def __init__(self, categories, iou_thresholds=(0.5,), recall_level=0.8, capacity=1 << 20, device='cuda:0', storage=None,
                 evaluate_corlocs=False, metric_prefix=None):
        if any(str(cat.get('name', '')).lower() == 'unknown' for cat in categories):
            raise ValueError("the unknown class is max(id) + 1 by itself: leave it out of `categories`")
        if len(set(cat['id'] for cat in categories)) != len(categories):
            raise ValueError('category ids must be distinct')
        self._num_known = max(cat['id'] for cat in categories)
        if self._num_known + 1 > 65535:
            raise ValueError('at most 65534 known classes (the unknown class is one of the 65535)')
        self._level = _check_level(recall_level)
        open_buf = None
        if storage is not None:
            if len(storage) != 4:
                raise ValueError('storage: (scores, classes, flags, open)')
            open_buf, storage = storage[3], tuple(storage[:3])
        known = list(categories)
        super().__init__(known + [{'id': self._num_known + 1, 'name': 'unknown'}], iou_thresholds=iou_thresholds, capacity=capacity,
                         evaluate_corlocs=evaluate_corlocs, metric_prefix=metric_prefix, device=device, storage=storage)
        self._categories = known
        if open_buf is not None:
            if open_buf.device != self.device or open_buf.dtype != torch.int32 or open_buf.dim() != 1 \
                    or not open_buf.is_contiguous() or open_buf.numel() < self.capacity:
                raise ValueError('storage: contiguous 1-d float32 / int32 / int32 / int32 GPU tensors of at least the capacity')
            self._open = open_buf[:self.capacity]
        else:
            self._open = torch.empty(self.capacity, dtype=torch.int32, device=self.device)

    @property
    def unknown_class(self):
        return self._num_known + 1

    def _alloc_blocks(self, T, C, dev):
        self._ws = torch.empty(self.lib.effdet_eval_open_sorted_workspace_bytes(self.capacity, C) // 8, dtype=torch.int64, device=dev)
        self._result = torch.zeros(self.lib.effdet_eval_open_sorted_result_bytes(T, C) // 8, dtype=torch.int64, device=dev)

    def add_batch(self, det, count, gt_boxes, gt_cls, gt_difficult=None):
        """As `DatasetDetectionEvaluator.add_batch` with classes 1..C + 1.  -> (flag words, open words) [B, max_det] int32: bit t of
        the open word = a kept known-class detection whose largest IoU with the image's unknown boxes is >= threshold t."""
        det, flags, kept, gt_boxes, gt_cls = self._match(det, count, gt_boxes, gt_cls, gt_difficult)
        B, max_det, _ = det.shape
        M = gt_boxes.shape[1]
        st = self._st()
        open_words = torch.empty(B, max_det, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.effdet_eval_open_words(st, det.data_ptr(), flags.data_ptr(), gt_boxes.data_ptr(), gt_cls.data_ptr(), B,
                                                   max_det, M, self._num_classes, self._thr, len(self._thresholds),
                                                   open_words.data_ptr()), 'effdet_eval_open_words')
        _lib.check(self.lib.effdet_eval_append_open(st, det.data_ptr(), flags.data_ptr(), open_words.data_ptr(), kept.data_ptr(), B,
                                                    max_det, self._bufs[0].data_ptr(), self._bufs[1].data_ptr(),
                                                    self._bufs[2].data_ptr(), self._open.data_ptr(), self.capacity,
                                                    self._state.data_ptr()), 'effdet_eval_append_open')
        return flags, open_words

    def enqueue(self, recall_level=None):
        """Sort + AP + open-set counts into the result block on the device; no host synchronisation."""
        level = self._level if recall_level is None else _check_level(recall_level)
        self._flush_pending()
        _lib.check(self.lib.effdet_eval_open_sorted(
            self._st(), self._bufs[0].data_ptr(), self._bufs[1].data_ptr(), self._bufs[2].data_ptr(), self._open.data_ptr(),
            self.capacity, -1, self._state.data_ptr(), len(self._thresholds), self._num_classes, self._gt_count.data_ptr(),
            self._gt_imgs.data_ptr(), self._correct.data_ptr(), level, self._ws.data_ptr(), self._ws.numel() * 8,
            self._result.data_ptr()), 'effdet_eval_open_sorted')

    def result(self):
        """The result block of the last `enqueue()` (ONE device-to-host copy) -> the dict of `DatasetDetectionEvaluator.result` over
        C + 1 classes (column C = the unknown class), the int64 matrices [T, C + 1] n_det, tp, open_total, k_star, pos, rank_at,
        open_at, tp_at, and the float64 metrics of `open_set_metrics`."""
        block = self._result.cpu()
        r = parse_open_result(block, len(self._thresholds), self._num_classes)
        if r['lost']:
            raise RuntimeError('%d detections were lost: more were added than the capacity of %d holds' % (r['lost'], self.capacity))
        r.update(open_set_metrics(r, self._num_known))
        r['block'] = block.numpy()
        return r

    def _sorted_offsets(self):
        return [self.lib.effdet_eval_open_sorted_offset(self.capacity, self._num_classes, w) for w in (0, 1, 2)]

    def evaluate(self, task_categories=None, batch_cats=None, recall_level=None):
        """`DatasetDetectionEvaluator.evaluate`'s keys over the KNOWN classes (mAP and mean CorLoc are their means; the same
        `metric_prefix`, CorLoc keys with `evaluate_corlocs`), and per threshold OpenSet/WI, OpenSet/A-OSE, OpenSet/U-Recall,
        OpenSet/U-Precision, OpenSet/U-AP and per-class Recall / Precision."""
        self.enqueue(recall_level)
        r = self.result()
        C = self._num_known
        ap = r['ap'][:, :C]
        with np.errstate(invalid='ignore', divide='ignore'):
            corloc = np.where(r['gt_imgs'][None, :C] == 0, np.nan, r['correct'][:, :C].astype(float) / r['gt_imgs'][None, :C])
        if task_categories is None:
            index = create_category_index(self._categories)
            task_categories = [index[i + 1]['name'] if i + 1 in index else 'class_%d' % (i + 1) for i in range(C)]
        nanmean = lambda v: float(np.nanmean(v)) if np.isfinite(v).any() else float('nan')
        out, maps = {}, []
        for t, thr in enumerate(self._thresholds):
            maps.append(nanmean(ap[t]))
            out[self._metric_prefix + 'Precision/mAP@{}IOU'.format(thr)] = maps[-1]
            if self._evaluate_corlocs:
                out[self._metric_prefix + 'Precision/meanCorLoc@{}IOU'.format(thr)] = nanmean(corloc[t])
            out['OpenSet/WI@{}IOU'.format(thr)] = float(r['wi'][t])
            out['OpenSet/A-OSE@{}IOU'.format(thr)] = int(r['a_ose'][t])
            out['OpenSet/U-Recall@{}IOU'.format(thr)] = float(r['u_recall'][t])
            out['OpenSet/U-Precision@{}IOU'.format(thr)] = float(r['u_precision'][t])
            out['OpenSet/U-AP@{}IOU'.format(thr)] = float(r['u_ap'][t])
            for idx, category_name in enumerate(task_categories):
                if batch_cats is not None and idx not in batch_cats:
                    continue
                out['AP@{}IOU/{}'.format(thr, category_name)] = ap[t, idx]
                if self._evaluate_corlocs:
                    out['CorLoc@{}IOU/{}'.format(thr, category_name)] = corloc[t, idx]
                out['Recall@{}IOU/{}'.format(thr, category_name)] = r['recall'][t, idx]
                out['Precision@{}IOU/{}'.format(thr, category_name)] = r['precision'][t, idx]
        if len(self._thresholds) > 1:
            out[self._metric_prefix + 'Precision/mAP@[{}:{}]IOU'.format(self._thresholds[0], self._thresholds[-1])] = nanmean(np.array(maps))
        return out
