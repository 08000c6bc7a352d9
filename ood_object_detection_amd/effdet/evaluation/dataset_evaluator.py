"""Detection evaluation over a whole validation set on the device (csrc/eval_scale.hip): the PASCAL-style mAP / CorLoc of
`ObjectDetectionEvaluator` (the reference's VOC all-points AP, effdet/evaluation/metrics.py:4-90) for up to 2^24 accumulated
detections, at up to 16 IoU thresholds from ONE matching pass and ONE sort, with `difficult` ground truth.

`add_batch` takes the `[B, max_det, 6]` detections + counts of `DetBenchPredict` as they come: one matching launch (a workgroup
per image, all thresholds), then the valid rows go to capacity-sized device buffers at a cursor that lives on the device.
`enqueue()` sorts (class, score descending, equal scores in arrival order) and computes AP per (threshold, class); `result()`
is the one device-to-host copy.  Nothing before `result()` synchronises with the host, so `add_batch` and `enqueue` can be
captured in a `torch.cuda.graph`; the same images give the same bits however they are split into `add_batch` calls.  No CPU
fallback.  Group-of boxes, their weight, verified image-level labels and the weighted (pooled) mAP are the subclasses of
openimages_evaluator.py (csrc/openimages_eval.hip); this class still raises for `group_of`.  Not built (they raise): masks, full
precision / recall curves, recall bounds.  The precision at ONE recall level, per-class recall / precision and the open-set
metrics are in open_set_evaluator.py.
"""
import ctypes

import numpy as np
import torch

from ... import _lib
from .detection_evaluator import SingleImageAPI, create_category_index

MAX_DETECTIONS = 1 << 24
MAX_THRESHOLDS = 16
RESULT_HEAD = 8                      # 8-byte words in front of the AP matrix: n, lost, NaN scores, T, C, 0, 0, 0


def _check_thresholds(iou_thresholds):
    thr = [float(t) for t in iou_thresholds]
    if not 1 <= len(thr) <= MAX_THRESHOLDS:
        raise ValueError('1 to %d IoU thresholds, got %d' % (MAX_THRESHOLDS, len(thr)))
    if any(not b > a for a, b in zip(thr, thr[1:])) or any(t != t for t in thr):
        raise ValueError('IoU thresholds must ascend, got %r' % (thr,))
    return thr


def sorted_ap(lib, stream, scores, classes, flags, n, num_thresholds, num_classes, gt_count, gt_imgs, correct, state=None,
              workspace=None, result=None):
    """effdet_eval_ap_sorted over float32 scores / int32 0-based classes / int32 flag words (1-d, contiguous, equally long = the
    capacity).  n: entries to use, or None to take the count from the device cursor `state[0]`.  -> the result block (int64)."""
    capacity = scores.numel()
    nb = lib.effdet_eval_ap_sorted_workspace_bytes(capacity, num_classes)
    rb = lib.effdet_eval_ap_sorted_result_bytes(num_thresholds, num_classes)
    if nb <= 0 or rb <= 0:
        raise ValueError('effdet_eval_ap_sorted: capacity in [1, 2^24], classes in [1, 65535], thresholds in [1, 16] '
                         '(got %d, %d, %d)' % (capacity, num_classes, num_thresholds))
    if workspace is None:
        workspace = torch.empty(nb // 8, dtype=torch.int64, device=scores.device)
    if result is None:
        result = torch.zeros(rb // 8, dtype=torch.int64, device=scores.device)
    _lib.check(lib.effdet_eval_ap_sorted(stream, scores.data_ptr(), classes.data_ptr(), flags.data_ptr(), capacity,
                                         -1 if n is None else n, state.data_ptr() if state is not None else None,
                                         num_thresholds, num_classes, gt_count.data_ptr(), gt_imgs.data_ptr(), correct.data_ptr(),
                                         workspace.data_ptr(), workspace.numel() * 8, result.data_ptr()), 'effdet_eval_ap_sorted')
    return result


def parse_result(block, T, C):
    """the host copy of a result block -> dict(n, lost, nan_scores, ap [T, C] float64, gt_count [C], gt_imgs [C], correct [T, C])"""
    w = block.numpy() if torch.is_tensor(block) else np.asarray(block)
    assert int(w[3]) == T and int(w[4]) == C
    o = RESULT_HEAD
    ap = w[o:o + T * C].view(np.float64).reshape(T, C).copy()
    o += T * C
    return dict(n=int(w[0]), lost=int(w[1]), nan_scores=int(w[2]), ap=ap, gt_count=w[o:o + C].copy(),
                gt_imgs=w[o + C:o + 2 * C].copy(), correct=w[o + 2 * C:o + 2 * C + T * C].reshape(T, C).copy())


class DatasetDetectionEvaluator(SingleImageAPI):
    """categories: [{'id': 1-based, 'name': ...}].  capacity: the most detections held between `clear()` calls (<= 2^24); more are
    counted and `result()` raises.  storage: optional caller-owned (scores float32, classes int32, flags int32) 1-d GPU tensors of
    at least `capacity` entries to accumulate in."""

    def __init__(self, categories, iou_thresholds=(0.5,), capacity=1 << 20, evaluate_corlocs=False, metric_prefix=None,
                 device='cuda:0', storage=None):
        self._categories = categories
        self._num_classes = max(cat['id'] for cat in categories)
        if min(cat['id'] for cat in categories) < 1:
            raise ValueError('Classes should be 1-indexed.')
        if self._num_classes > 65535:
            raise ValueError('at most 65535 classes')
        self._thresholds = _check_thresholds(iou_thresholds)
        self.capacity = int(capacity)
        if not 1 <= self.capacity <= MAX_DETECTIONS:
            raise ValueError('capacity must lie in [1, 2^24], got %d' % self.capacity)
        self._evaluate_corlocs = evaluate_corlocs
        self._metric_prefix = (metric_prefix + '_') if metric_prefix else ''
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('the evaluator runs on the GPU (no CPU fallback)')
        self.lib = _lib.load()
        T, C, dev = len(self._thresholds), self._num_classes, self.device
        self._thr = (ctypes.c_float * T)(*self._thresholds)
        if storage is not None:
            scores, classes, flags = storage
            for b, dt in ((scores, torch.float32), (classes, torch.int32), (flags, torch.int32)):
                if b.device != dev or b.dtype != dt or b.dim() != 1 or not b.is_contiguous() or b.numel() < self.capacity:
                    raise ValueError('storage: contiguous 1-d float32 / int32 / int32 GPU tensors of at least the capacity')
            self._bufs = (scores[:self.capacity], classes[:self.capacity], flags[:self.capacity])
        else:
            self._bufs = (torch.empty(self.capacity, dtype=torch.float32, device=dev),
                          torch.empty(self.capacity, dtype=torch.int32, device=dev),
                          torch.empty(self.capacity, dtype=torch.int32, device=dev))
        self._alloc_blocks(T, C, dev)
        self._state = torch.zeros(4, dtype=torch.int32, device=dev)          # cursor, lost, NaN scores, 0
        self._counters = torch.zeros(2 * C + T * C, dtype=torch.int32, device=dev)
        self._gt_count, self._gt_imgs, self._correct = self._counters[:C], self._counters[C:2 * C], self._counters[2 * C:]
        self._reset_host()

    def _alloc_blocks(self, T, C, dev):
        self._ws = torch.empty(self.lib.effdet_eval_ap_sorted_workspace_bytes(self.capacity, C) // 8, dtype=torch.int64, device=dev)
        self._result = torch.zeros(self.lib.effdet_eval_ap_sorted_result_bytes(T, C) // 8, dtype=torch.int64, device=dev)

    def _reset_host(self):
        self._pending_gt = {}
        self._seen_det = set()
        self._image_ids = set()

    def _accepts_difficult(self):
        return True

    def _st(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def clear(self):
        """Forget everything (cursor and counters are reset on the device, no synchronisation)."""
        self._state.zero_()
        self._counters.zero_()
        self._reset_host()

    def add_batch(self, det, count, gt_boxes, gt_cls, gt_difficult=None):
        """det [B, max_det, 6] rows x1,y1,x2,y2,score,class (1-based) in descending score order, `count[b]` valid rows; gt_boxes
        [B, M, 4] yxyx, gt_cls [B, M] 1-based (<= 0: padding), gt_difficult [B, M] bool or None.  -> flag words [B, max_det] int32:
        bit t = true positive at threshold t, bit 16 + t = ignored there, bit 31 (negative) = dropped."""
        det, flags, kept, _, _ = self._match(det, count, gt_boxes, gt_cls, gt_difficult)
        B, max_det, _ = det.shape
        _lib.check(self.lib.effdet_eval_append(self._st(), det.data_ptr(), flags.data_ptr(), kept.data_ptr(), B, max_det,
                                               self._bufs[0].data_ptr(), self._bufs[1].data_ptr(), self._bufs[2].data_ptr(),
                                               self.capacity, self._state.data_ptr()), 'effdet_eval_append')
        return flags

    def _match(self, det, count, gt_boxes, gt_cls, gt_difficult):
        """the matching launch of `add_batch` -> (det, flags, kept [2 B], gt_boxes, gt_cls) as the device saw them"""
        dev = self.device
        det = det.to(device=dev, dtype=torch.float32).contiguous()
        count = count.to(device=dev, dtype=torch.int32).contiguous()
        gt_boxes = gt_boxes.to(device=dev, dtype=torch.float32).contiguous()
        gt_cls = gt_cls.to(device=dev, dtype=torch.int64).contiguous()
        B, max_det, _ = det.shape
        M = gt_boxes.shape[1]
        if M == 0:
            gt_boxes = torch.zeros(B, 1, 4, dtype=torch.float32, device=dev)
            gt_cls = torch.zeros(B, 1, dtype=torch.int64, device=dev)
            gt_difficult, M = None, 1
        if gt_difficult is not None:
            gt_difficult = gt_difficult.to(device=dev, dtype=torch.uint8).contiguous()
            if tuple(gt_difficult.shape) != (B, M):
                raise ValueError('gt_difficult must be [B, M]')
        flags = torch.empty(B, max_det, dtype=torch.int32, device=dev)
        kept = torch.empty(2 * B, dtype=torch.int32, device=dev)
        self._launch_match(det, count, gt_boxes, gt_cls, gt_difficult.data_ptr() if gt_difficult is not None else None, B, max_det, M,
                           flags, kept)
        return det, flags, kept, gt_boxes, gt_cls

    def _launch_match(self, det, count, gt_boxes, gt_cls, gt_difficult_ptr, B, max_det, M, flags, kept):
        """the matching launch itself on prepared device tensors (a subclass with its own entry point overrides this)"""
        _lib.check(self.lib.effdet_eval_match_multi(self._st(), det.data_ptr(), count.data_ptr(), gt_boxes.data_ptr(), gt_cls.data_ptr(),
                                                    gt_difficult_ptr, B, max_det, M, self._num_classes, self._thr,
                                                    len(self._thresholds), flags.data_ptr(), kept.data_ptr(), self._gt_count.data_ptr(),
                                                    self._gt_imgs.data_ptr(), self._correct.data_ptr()), 'effdet_eval_match_multi')

    def enqueue(self):
        """Sort + metrics into the result block on the device; no host synchronisation."""
        self._flush_pending()
        T, C = len(self._thresholds), self._num_classes
        sorted_ap(self.lib, self._st(), self._bufs[0], self._bufs[1], self._bufs[2], None, T, C, self._gt_count, self._gt_imgs,
                  self._correct, state=self._state, workspace=self._ws, result=self._result)

    def result(self):
        """The result block of the last `enqueue()` (ONE device-to-host copy) -> dict(n, lost, nan_scores, ap [T, C], gt_count,
        gt_imgs, correct [T, C], block: the raw int64 words)."""
        block = self._result.cpu()
        r = parse_result(block, len(self._thresholds), self._num_classes)
        if r['lost']:
            raise RuntimeError('%d detections were lost: more were added than the capacity of %d holds' % (r['lost'], self.capacity))
        r['block'] = block.numpy()
        return r

    def _sorted_offsets(self):
        return [self.lib.effdet_eval_ap_sorted_offset(self.capacity, self._num_classes, w) for w in (0, 1)]

    def sorted(self):
        """After `enqueue()`: (class [n] int64, score [n] float32, flag word [n] uint32) of the valid entries in the sorted order
        (debug / test accessor; synchronises)."""
        C = self._num_classes
        ws = self._ws.view(torch.uint8)
        offs = self._sorted_offsets()
        ko = offs[0]
        n = min(int(self._state[0].item()), self.capacity)
        keys = ws[ko:ko + 8 * n].cpu().numpy().view(np.uint64)
        words = [ws[o:o + 4 * n].cpu().numpy().view(np.uint32) for o in offs[1:]]
        cls = (keys >> np.uint64(32)).astype(np.int64)
        k = ~(keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)                 # the order-preserving map of the float32 bits
        bits = np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k)
        valid = cls < C
        return (cls[valid], bits.view(np.float32)[valid]) + tuple(w[valid] for w in words)

    def evaluate(self, task_categories=None, batch_cats=None):
        """Metric dict with the reference's keys (detection_evaluator.py:268-305) at every threshold, and with more than one
        threshold 'Precision/mAP@[first:last]IOU' = the mean of the per-threshold mAPs that are not NaN."""
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
            maps.append(nanmean(ap[t]))
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
