"""LVIS federated detection evaluation on the device (csrc/lvis_eval.hip): what lvis-api's `LVISEval(gt, dt, 'bbox')` computes.
LVIS annotates an image exhaustively only for the categories of its positive set and checks it for absence only of those of its
negative set: a detection of any other category is neither a true nor a false positive there, an unmatched detection of a category
that is `not exhaustive` in the image is ignored, and the cap of 300 detections an image runs over ALL categories.

`add_batch` takes the `[B, max_det, 6]` detections + counts of `DetBenchPredict` with the rows in any order, and per image the
padded category lists `neg_cls` (checked absent) and `nel_cls` (not exhaustively annotated): one matching launch (a workgroup per
image ranks its detections, cuts at `max_dets[-1]`, filters by the image's category sets and matches in rank order), then the
append of `CocoDetectionEvaluator`.  `enqueue`, `result`, `precision`, `sorted`, `clear`, the capacity, the overflow report and
the `storage` option are that class's own: the accumulate stage of LVIS is COCO's.  `evaluate()` names the thirteen LVIS figures;
`APr`, `APc`, `APf` are means over the categories whose `frequency` is 'r', 'c' or 'f'.  The per-episode `evaluate(task_categories,
batch_cats)` of the few-shot code is this protocol with the task's categories as every image's `neg_cls`.  No CPU fallback.  Not
built: masks, crowd regions (LVIS has none), merging evaluators across ranks on the device.
"""
import numpy as np
import torch

from ... import _lib
from .coco_evaluator import COCO_AREA_LABELS, COCO_AREA_RANGES, CocoDetectionEvaluator

MAX_DET = 2048                       # the most detection slots an image may have (LV_MAX_DET of csrc/lvis_eval.hip)
LVIS_FIGURES = ('AP', 'AP50', 'AP75', 'APs', 'APm', 'APl', 'APr', 'APc', 'APf', 'AR@%d', 'ARs@%d', 'ARm@%d', 'ARl@%d')


class LvisDetectionEvaluator(CocoDetectionEvaluator):
    """categories: [{'id': 1-based, 'name': ..., 'frequency': 'r' | 'c' | 'f' (optional)}].  The other arguments are those of
    `CocoDetectionEvaluator`; `max_dets` defaults to LVIS's (300,) and its last entry is the cap over all categories of an image."""

    def __init__(self, categories, iou_thresholds=np.linspace(.5, .95, 10), area_ranges=COCO_AREA_RANGES, max_dets=(300,),
                 recall_thresholds=np.linspace(0, 1, 101), min_score=0.0, capacity=1 << 20, keep_precision=False, device='cuda:0',
                 storage=None, area_labels=COCO_AREA_LABELS):
        super().__init__(categories, iou_thresholds=iou_thresholds, area_ranges=area_ranges, max_dets=max_dets,
                         recall_thresholds=recall_thresholds, min_score=min_score, capacity=capacity, keep_precision=keep_precision,
                         device=device, storage=storage, area_labels=area_labels)

    def _category_list(self, t, B, name):
        """[B, K] int64 on the device, or None; K = 0 (the empty set) becomes one column of padding: its pointer is not null"""
        if t is None:
            return None
        t = t.to(device=self.device, dtype=torch.int64).contiguous()
        if t.dim() != 2 or t.shape[0] != B:
            raise ValueError('%s must be [B, K]' % name)
        return t if t.shape[1] else torch.zeros(B, 1, dtype=torch.int64, device=self.device)

    def add_batch(self, det, count, gt_boxes, gt_cls, gt_area=None, neg_cls=None, nel_cls=None):
        """det [B, max_det, 6] rows x1,y1,x2,y2,score,class (1-based) in any order, `count[b]` valid rows (max_det <= 2048);
        gt_boxes [B, M, 4] yxyx, gt_cls [B, M] 1-based (<= 0: padding), gt_area [B, M] float32 or None (the box area); neg_cls
        [B, Kn] / nel_cls [B, Ke] int64 1-based categories (<= 0: padding) checked absent / not exhaustively annotated in the image
        (None: every category is judged in every image / no category is not-exhaustive).  -> flag words [B, max_det, A] int32: bit
        t = true positive at threshold t, bit 16 + t = ignored there, bit 31 (negative) = dropped."""
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
        if M == 0:
            gt_boxes = torch.zeros(B, 1, 4, dtype=torch.float32, device=dev)
            gt_cls = torch.zeros(B, 1, dtype=torch.int64, device=dev)
            gt_area, M = None, 1
        if gt_area is not None:
            gt_area = gt_area.to(device=dev, dtype=torch.float32).contiguous()
            if tuple(gt_area.shape) != (B, M):
                raise ValueError('gt_area must be [B, M]')
        neg_cls, nel_cls = self._category_list(neg_cls, B, 'neg_cls'), self._category_list(nel_cls, B, 'nel_cls')
        A = len(self._areas)
        flags = torch.empty(B, max_det, A, dtype=torch.int32, device=dev)
        rank = torch.empty(B, max_det, dtype=torch.int32, device=dev)
        kept = torch.empty(2 * B, dtype=torch.int32, device=dev)
        st = self._st()
        _lib.check(self.lib.effdet_lvis_match(st, det.data_ptr(), count.data_ptr(), gt_boxes.data_ptr(), gt_cls.data_ptr(),
                                              gt_area.data_ptr() if gt_area is not None else None, B, max_det, M, self._num_classes,
                                              self._thr, len(self._thresholds), self._area_arr, A, self._max_dets[-1], self.min_score,
                                              neg_cls.data_ptr() if neg_cls is not None else None,
                                              neg_cls.shape[1] if neg_cls is not None else 0,
                                              nel_cls.data_ptr() if nel_cls is not None else None,
                                              nel_cls.shape[1] if nel_cls is not None else 0,
                                              flags.data_ptr(), rank.data_ptr(), kept.data_ptr(), self._npig.data_ptr()),
                   'effdet_lvis_match')
        _lib.check(self.lib.effdet_coco_append(st, det.data_ptr(), flags.data_ptr(), rank.data_ptr(), kept.data_ptr(), B, max_det, A,
                                               self._bufs[0].data_ptr(), self._bufs[1].data_ptr(), self._bufs[2].data_ptr(),
                                               self._bufs[3].data_ptr(), self.capacity, self._state.data_ptr()), 'effdet_coco_append')
        self._last_rank = rank
        return flags

    # ---- host glue: LVISEval.summarize ----------------------------------------------------------------------------------------
    def _group_mean(self, ap, freq):
        """mean of AP over the thresholds and the categories of one frequency group (area 'all', the largest max_dets); -1
        without a category in the group, without `frequency` in the categories, or without a cell that is not NaN"""
        cls = [cat['id'] - 1 for cat in self._categories if cat.get('frequency') == freq]
        if not cls or 'all' not in self._area_labels:
            return -1.0
        s = ap[:, cls, self._area_labels.index('all'), len(self._max_dets) - 1]
        s = s[~np.isnan(s)]
        return float(np.mean(s)) if s.size else -1.0

    def evaluate(self):
        """`enqueue()` + `result()` -> dict with the thirteen LVIS figures ('AP', 'AP50', 'AP75', 'APs', 'APm', 'APl', 'APr',
        'APc', 'APf', 'AR@300', 'ARs@300', 'ARm@300', 'ARl@300': means over the cells that are not NaN, -1 where there is none;
        300 = the largest max_dets), 'AP/<name>' per class (area 'all', NaN without ground truth) and 'stats': the thirteen in
        this order."""
        self.enqueue()
        r = self.result()
        ap, ar = r['ap'], r['ar']
        last = len(self._max_dets) - 1
        md = self._max_dets[last]
        values = [self._mean(ap, None, 'all', last), self._mean(ap, 0.5, 'all', last), self._mean(ap, 0.75, 'all', last),
                  self._mean(ap, None, 'small', last), self._mean(ap, None, 'medium', last), self._mean(ap, None, 'large', last),
                  self._group_mean(ap, 'r'), self._group_mean(ap, 'c'), self._group_mean(ap, 'f'),
                  self._mean(ar, None, 'all', last), self._mean(ar, None, 'small', last), self._mean(ar, None, 'medium', last),
                  self._mean(ar, None, 'large', last)]
        out = {(k % md if '%d' in k else k): v for k, v in zip(LVIS_FIGURES, values)}
        names = {cat['id']: cat['name'] for cat in self._categories}
        a_all = self._area_labels.index('all') if 'all' in self._area_labels else 0
        for c in range(self._num_classes):
            v = ap[:, c, a_all, last]
            v = v[~np.isnan(v)]
            out['AP/%s' % names.get(c + 1, str(c + 1))] = float(np.mean(v)) if v.size else float('nan')
        out['stats'] = np.array(values)
        self.stats = out['stats']
        return out
