"""Detection calibration on the device (csrc/calibration_eval.hip): does a detection's score mean what it says?  Reliability tables
of the score under the PASCAL matching of `DatasetDetectionEvaluator` (the same flag words and counters, `difficult` boxes
ignored), on its storage, `enqueue`, `result` and `clear`, at up to 16 IoU thresholds from one matching pass.

`add_batch` matches and appends (score, class, flag word, IoU with the candidate box) of the kept detections; a detection below
`score_threshold` still takes its box and is then left out.  `enqueue()` sorts by (class, score descending) and once more by score
alone (the `pooled` scope) and fills, per (threshold, scope, binning scheme, bin), n, tp, the sum of the scores and the sum of the
IoU over the true positives, in float64 and in an order that depends on the sorted positions alone: the same images give the same
bits from run to run and for every split into batches, nothing synchronises with the host before `result()`, and `add_batch` +
`enqueue` can be captured.  `evaluate()` is float64 host glue over the tables:

  D-ECE          Kueppers et al. 2020, confidence only: pooled scope, equal-width bins, sum_k (n_k / n) |conf_k - prec_k|
  MCE            the largest bin gap of the same table
  ACE            the same sum over equal-mass bins (bin k = sorted positions [floor(k m / K), floor((k + 1) m / K)))
  classwise-ECE  the mean of the per-class equal-width sum over the classes with entries
  LaECE          Oksuz et al. 2023: the mean over the classes with entries of sum_k (n_k / n_c) |conf_k - sum_iou_k / n_k|
  Brier, NLL     the means of (p - tp)^2 and of -log(tp ? p~ : 1 - p~), p~ = p clamped to [2^-24, 1 - 2^-24], pooled

Not built: the box-position and box-size dimensions of D-ECE, histogram-binning and isotonic calibrators (they are not monotone in
float32 and would break the score order the evaluators need; the monotone Platt / temperature calibrator is
`ood_object_detection_amd.calibration.DetectionCalibrator`), per-class calibrators.  No CPU fallback.
"""
import ctypes

import numpy as np
import torch

from ... import _lib
from .dataset_evaluator import RESULT_HEAD, DatasetDetectionEvaluator

MAX_BINS = 64
MAX_CELLS = 1 << 20                  # thresholds * (classes + 1) * bins of one result block
SCHEMES = ('width', 'mass')


def parse_calibration_result(block, T, C, K):
    """the host copy of a result block -> dict(n, lost, nan_scores, bins: dict(n, tp [T, C + 1, 2, K] int64, sum_p, sum_iou the same
    in float64), brier, nll [T, C + 1] float64, out_of_range, entries [T, C + 1] int64, gt_count [C], gt_imgs [C], correct [T, C]);
    scope C is `pooled`, scheme 0 is `width`, 1 is `mass`"""
    w = block.numpy() if torch.is_tensor(block) else np.asarray(block)
    assert int(w[3]) == T and int(w[4]) == C and int(w[5]) == K
    S = C + 1
    cells, o = T * S * 2 * K, RESULT_HEAD
    take = lambda n, shape, dt: w[n:n + int(np.prod(shape))].view(dt).reshape(shape).copy()
    bins = dict(n=take(o, (T, S, 2, K), np.int64), tp=take(o + cells, (T, S, 2, K), np.int64),
                sum_p=take(o + 2 * cells, (T, S, 2, K), np.float64), sum_iou=take(o + 3 * cells, (T, S, 2, K), np.float64))
    o += 4 * cells
    out = dict(n=int(w[0]), lost=int(w[1]), nan_scores=int(w[2]), bins=bins, brier=take(o, (T, S), np.float64),
               nll=take(o + T * S, (T, S), np.float64), out_of_range=take(o + 2 * T * S, (T, S), np.int64),
               entries=take(o + 3 * T * S, (T, S), np.int64))
    o += 4 * T * S
    out.update(gt_count=w[o:o + C].copy(), gt_imgs=w[o + C:o + 2 * C].copy(), correct=w[o + 2 * C:o + 2 * C + T * C].reshape(T, C).copy())
    return out


def bin_gaps(n, conf_sum, target_sum):
    """one (threshold, scope, scheme) row of the tables: n [K] int, the two sums [K] float64 -> (sum_k (n_k / n) gap_k, max gap,
    gaps [K] with NaN in the empty bins), gap_k = |conf_sum_k / n_k - target_sum_k / n_k|; (NaN, NaN) without entries"""
    K, total = len(n), int(np.sum(n))
    gaps = np.full(K, np.nan)
    if total == 0:
        return float('nan'), float('nan'), gaps
    ece, mce = 0.0, 0.0
    for k in range(K):
        if n[k] == 0:
            continue
        nk = float(n[k])
        gap = abs(float(conf_sum[k]) / nk - float(target_sum[k]) / nk)
        gaps[k] = gap
        ece = ece + (nk / float(total)) * gap
        mce = max(mce, gap)
    return ece, mce, gaps


def calibration_metrics(r, t):
    """the metrics at threshold index t from a parsed result block (float64 host glue; tests/_calibration_ref.py restates it)"""
    b = r['bins']
    C = b['n'].shape[1] - 1
    d_ece, mce, _ = bin_gaps(b['n'][t, C, 0], b['sum_p'][t, C, 0], b['tp'][t, C, 0])
    ace, _, _ = bin_gaps(b['n'][t, C, 1], b['sum_p'][t, C, 1], b['tp'][t, C, 1])
    cw, la = [], []
    for c in range(C):
        if int(b['n'][t, c, 0].sum()) == 0:
            continue
        cw.append(bin_gaps(b['n'][t, c, 0], b['sum_p'][t, c, 0], b['tp'][t, c, 0])[0])
        la.append(bin_gaps(b['n'][t, c, 0], b['sum_p'][t, c, 0], b['sum_iou'][t, c, 0])[0])
    n = int(b['n'][t, C, 0].sum())
    mean = lambda v: float(np.sum(np.asarray(v, np.float64)) / len(v)) if v else float('nan')
    return {'D-ECE': d_ece, 'MCE': mce, 'ACE': ace, 'classwise-ECE': mean(cw), 'LaECE': mean(la),
            'Brier': float(r['brier'][t, C]) / n if n else float('nan'), 'NLL': float(r['nll'][t, C]) / n if n else float('nan'),
            'n': n, 'out_of_range': int(r['out_of_range'][t, C])}


def reliability_diagram(r, t, scope=None, scheme='width'):
    """per-bin (mean confidence, precision, mean IoU of the true positives, count) of one scope (None: pooled); NaN where a bin is
    empty (the mean IoU: where it has no true positive)"""
    b = r['bins']
    s = b['n'].shape[1] - 1 if scope is None else scope
    z = SCHEMES.index(scheme)
    n, tp = b['n'][t, s, z].astype(np.float64), b['tp'][t, s, z].astype(np.float64)
    with np.errstate(invalid='ignore', divide='ignore'):
        return dict(confidence=np.where(n > 0, b['sum_p'][t, s, z] / n, np.nan), precision=np.where(n > 0, tp / n, np.nan),
                    iou=np.where(tp > 0, b['sum_iou'][t, s, z] / tp, np.nan), count=b['n'][t, s, z].copy())


def check_calibration_shape(num_thresholds, num_classes, bins):
    if not 1 <= int(bins) <= MAX_BINS:
        raise ValueError('bins must lie in [1, %d], got %r' % (MAX_BINS, bins))
    if num_thresholds * (num_classes + 1) * int(bins) > MAX_CELLS:
        raise ValueError('thresholds * (classes + 1) * bins = %d exceeds %d' % (num_thresholds * (num_classes + 1) * int(bins), MAX_CELLS))


class CalibrationEvaluator(DatasetDetectionEvaluator):
    """categories, iou_thresholds (1 to 16, ascending), capacity, device: as DatasetDetectionEvaluator.  bins: 1 to 64.
    score_threshold: detections below it are matched and then left out.  storage: optional caller-owned (scores float32, classes
    int32, flags int32, iou float32) 1-d GPU tensors of at least `capacity` entries."""

    def __init__(self, categories, iou_thresholds=(0.5,), bins=15, score_threshold=0.0, capacity=1 << 20, metric_prefix=None,
                 device='cuda:0', storage=None):
        thr = list(iou_thresholds)
        check_calibration_shape(max(len(thr), 1), max(cat['id'] for cat in categories), bins)
        self._bins = int(bins)
        self._score_threshold = float(score_threshold)
        if self._score_threshold != self._score_threshold:
            raise ValueError('score_threshold is NaN')
        iou = None
        if storage is not None:
            if len(storage) != 4:
                raise ValueError('storage: (scores float32, classes int32, flags int32, iou float32)')
            storage, iou = tuple(storage[:3]), storage[3]
        super().__init__(categories, iou_thresholds=thr, capacity=capacity, evaluate_corlocs=False, metric_prefix=metric_prefix,
                         device=device, storage=storage)
        if iou is not None:
            if iou.device != self.device or iou.dtype != torch.float32 or iou.dim() != 1 or not iou.is_contiguous() \
                    or iou.numel() < self.capacity:
                raise ValueError('storage: contiguous 1-d float32 / int32 / int32 / float32 GPU tensors of at least the capacity')
            self._iou = iou[:self.capacity]
        else:
            self._iou = torch.empty(self.capacity, dtype=torch.float32, device=self.device)
        self._metric_names = [self._metric_prefix + 'Calibration/D-ECE@{}IOU'.format(self._thresholds[0])]
        self._last_iou = None

    def _alloc_blocks(self, T, C, dev):
        nb = self.lib.effdet_calibration_workspace_bytes(self.capacity, C)
        rb = self.lib.effdet_calibration_result_bytes(T, C, self._bins)
        if nb <= 0 or rb <= 0:
            raise ValueError('capacity %d, %d thresholds, %d classes, %d bins exceed the limits' % (self.capacity, T, C, self._bins))
        self._ws = torch.empty(nb // 8, dtype=torch.int64, device=dev)
        self._result = torch.zeros(rb // 8, dtype=torch.int64, device=dev)

    @property
    def bins(self):
        return self._bins

    @property
    def thresholds(self):
        return list(self._thresholds)

    def entries(self):
        """(scores, classes, flag words, IoU, state) of the appended, unsorted entries: the device buffers `DetectionCalibrator.fit`
        reads; state[0] is the live count"""
        return self._bufs[0], self._bufs[1], self._bufs[2], self._iou, self._state

    # ---- native entry -------------------------------------------------------------------------------------------------------------
    def add_batch(self, det, count, gt_boxes, gt_cls, gt_difficult=None):
        """as DatasetDetectionEvaluator.add_batch (the same flag words come back); `self._last_iou` [B, max_det] float32: the IoU of
        every slot with its candidate box."""
        if det.dim() != 3 or det.shape[2] != 6 or gt_boxes.dim() != 3 or gt_boxes.shape[2] != 4:
            raise ValueError('det must be [B, max_det, 6] and gt_boxes [B, M, 4]')
        if gt_boxes.shape[0] != det.shape[0] or tuple(gt_cls.shape) != tuple(gt_boxes.shape[:2]) or count.numel() != det.shape[0]:
            raise ValueError('count [B], gt_boxes [B, M, 4] and gt_cls [B, M] must agree with det')
        det, flags, kept, _, _ = self._match(det, count, gt_boxes, gt_cls, gt_difficult)
        B, max_det, _ = det.shape
        _lib.check(self.lib.effdet_calibration_append(self._st(), det.data_ptr(), flags.data_ptr(), self._last_iou.data_ptr(),
                                                      kept.data_ptr(), B, max_det, self._score_threshold, self._bufs[0].data_ptr(),
                                                      self._bufs[1].data_ptr(), self._bufs[2].data_ptr(), self._iou.data_ptr(),
                                                      self.capacity, self._state.data_ptr()), 'effdet_calibration_append')
        return flags

    def _launch_match(self, det, count, gt_boxes, gt_cls, gt_difficult_ptr, B, max_det, M, flags, kept):
        """DatasetDetectionEvaluator._match's launch on this unit's entry point: the same flag words and counters, and the IoU"""
        iou = torch.empty(B, max_det, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.effdet_calibration_match(self._st(), det.data_ptr(), count.data_ptr(), gt_boxes.data_ptr(), gt_cls.data_ptr(),
                                                     gt_difficult_ptr, B, max_det, M, self._num_classes, self._thr,
                                                     len(self._thresholds), self._score_threshold, flags.data_ptr(), iou.data_ptr(),
                                                     kept.data_ptr(), self._gt_count.data_ptr(), self._gt_imgs.data_ptr(),
                                                     self._correct.data_ptr()), 'effdet_calibration_match')
        self._last_iou = iou

    def enqueue(self):
        """Both sorts + the tables into the result block on the device; no host synchronisation."""
        self._flush_pending()
        _lib.check(self.lib.effdet_calibration_table(self._st(), self._bufs[0].data_ptr(), self._bufs[1].data_ptr(),
                                                     self._bufs[2].data_ptr(), self._iou.data_ptr(), self.capacity, -1,
                                                     self._state.data_ptr(), len(self._thresholds), self._num_classes, self._bins,
                                                     self._gt_count.data_ptr(), self._gt_imgs.data_ptr(), self._correct.data_ptr(),
                                                     self._ws.data_ptr(), self._ws.numel() * 8, self._result.data_ptr()),
                   'effdet_calibration_table')

    def result(self):
        """The result block of the last `enqueue()` (ONE device-to-host copy) -> parse_calibration_result's dict and `block`, the
        raw int64 words."""
        block = self._result.cpu()
        r = parse_calibration_result(block, len(self._thresholds), self._num_classes, self._bins)
        if r['lost']:
            raise RuntimeError('%d detections were lost: more were added than the capacity of %d holds' % (r['lost'], self.capacity))
        r['block'] = block.numpy()
        return r

    def _sorted_offsets(self):
        return [self.lib.effdet_calibration_sorted_offset(self.capacity, self._num_classes, w) for w in (0, 1, 2)]

    def evaluate(self, task_categories=None, batch_cats=None):
        """Metric dict: per threshold '<prefix>Calibration/<metric>@<thr>IOU' for D-ECE, MCE, ACE, classwise-ECE, LaECE, Brier and NLL,
        and 'Reliability@<thr>IOU' = the pooled equal-width diagram (confidence, precision, iou, count per bin)."""
        self.enqueue()
        r = self.result()
        out = {}
        for t, thr in enumerate(self._thresholds):
            m = calibration_metrics(r, t)
            for k in ('D-ECE', 'MCE', 'ACE', 'classwise-ECE', 'LaECE', 'Brier', 'NLL'):
                out[self._metric_prefix + 'Calibration/{}@{}IOU'.format(k, thr)] = m[k]
            out['Reliability@{}IOU'.format(thr)] = reliability_diagram(r, t)
        return out
