"""COCO-protocol detection evaluation on the device (csrc/coco_eval.hip): what pycocotools' `COCOeval(gt, dt, 'bbox')` computes
- crowd regions, the four area ranges, the greedy rule per IoU threshold, 101-point interpolated AP, AR at maxDets 1 / 10 / 100 -
for up to 2^24 accumulated detections, from ONE matching pass and ONE sort.

`add_batch` takes the `[B, max_det, 6]` detections + counts of `DetBenchPredict` as they come: one matching launch (a workgroup per
image, every threshold and area range), then the kept rows go to capacity-sized device buffers at a cursor that lives on the
device.  `enqueue()` sorts (class, score descending, equal scores in arrival order) and computes AP and AR per (threshold, class,
area range, max_dets); `result()` is the one device-to-host copy.  Nothing before `result()` synchronises with the host, so
`add_batch` and `enqueue` can be captured in a `torch.cuda.graph`; the same images give the same bits however they are split into
`add_batch` calls.  The means over classes and thresholds (`evaluate()`, `stats`) are host arithmetic over the entries that are not
NaN (pycocotools: `> -1`).  No CPU fallback.  LVIS's federated rules are `LvisDetectionEvaluator` (lvis_evaluator.py).  Not built:
masks, keypoints, `useCats=0`, merging evaluators across ranks on the device.
"""
import ctypes

import numpy as np
import torch

from ... import _lib

MAX_DETECTIONS = 1 << 24
MAX_THRESHOLDS, MAX_AREAS, MAX_MAX_DETS, MAX_RECALL_THRESHOLDS = 15, 4, 4, 256
RESULT_HEAD = 8                      # 8-byte words in front of AP: n, lost, NaN scores, T, C, A, Mx, R
COCO_AREA_RANGES = ((0.0, 1e5 ** 2), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e5 ** 2))
COCO_AREA_LABELS = ('all', 'small', 'medium', 'large')


def parse_coco_result(block):
    """the host copy of a result block -> dict(n, lost, nan_scores, ap / ar [T, C, A, Mx] float64, npig [C, A])"""
    w = block.numpy() if torch.is_tensor(block) else np.asarray(block)
    T, C, A, Mx = (int(v) for v in w[3:7])
    cells, o = T * C * A * Mx, RESULT_HEAD
    ap = w[o:o + cells].view(np.float64).reshape(T, C, A, Mx).copy()
    ar = w[o + cells:o + 2 * cells].view(np.float64).reshape(T, C, A, Mx).copy()
    return dict(n=int(w[0]), lost=int(w[1]), nan_scores=int(w[2]), ap=ap, ar=ar,
                npig=w[o + 2 * cells:o + 2 * cells + C * A].reshape(C, A).copy())


def _ascending(name, values, lo, hi, cast):
    v = [cast(x) for x in values]
    if not lo <= len(v) <= hi:
        raise ValueError('%d to %d %s, got %d' % (lo, hi, name, len(v)))
    if any(x != x for x in v) or any(not b > a for a, b in zip(v, v[1:])):
        raise ValueError('%s must ascend, got %r' % (name, v))
    return v


class CocoDetectionEvaluator:
    """categories: [{'id': 1-based, 'name': ...}].  iou_thresholds: 1..15 ascending; area_ranges: 1..4 [lo, hi] (inclusive);
    max_dets: 1..4 ascending; recall_thresholds: 1..256 ascending float64.  min_score: detections below it are dropped.
    capacity: the most detections held between `clear()` calls (<= 2^24); more are counted and `result()` raises.
    keep_precision: also keep the precision table [T, R, C, A, Mx] (the PR curves) on the device: `precision()`.
    storage: optional caller-owned (scores float32 [cap], classes int32 [cap], words int32 [cap * A], ranks int32 [cap]) GPU tensors."""

    def __init__(self, categories, iou_thresholds=np.linspace(.5, .95, 10), area_ranges=COCO_AREA_RANGES, max_dets=(1, 10, 100),
                 recall_thresholds=np.linspace(0, 1, 101), min_score=0.0, capacity=1 << 20, keep_precision=False, device='cuda:0',
                 storage=None, area_labels=COCO_AREA_LABELS):
        self._categories = categories
        self._num_classes = max(cat['id'] for cat in categories)
        if min(cat['id'] for cat in categories) < 1:
            raise ValueError('Classes should be 1-indexed.')
        if self._num_classes > 65535:
            raise ValueError('at most 65535 classes')
        self._thresholds = _ascending('IoU thresholds', iou_thresholds, 1, MAX_THRESHOLDS, lambda x: float(np.float32(x)))
        self._max_dets = _ascending('max_dets', max_dets, 1, MAX_MAX_DETS, int)
        if self._max_dets[0] < 1:
            raise ValueError('max_dets must be positive')
        self._rec = np.array(_ascending('recall thresholds', recall_thresholds, 1, MAX_RECALL_THRESHOLDS, float), np.float64)
        self._areas = [(float(lo), float(hi)) for lo, hi in area_ranges]
        if not 1 <= len(self._areas) <= MAX_AREAS or any(not lo <= hi for lo, hi in self._areas):
            raise ValueError('1 to %d area ranges [lo, hi] with lo <= hi, got %r' % (MAX_AREAS, self._areas))
        self._area_labels = tuple(area_labels)[:len(self._areas)]
        if len(self._area_labels) != len(self._areas):
            raise ValueError('an area label per area range')
        self.min_score = float(min_score)
        if self.min_score != self.min_score:
            raise ValueError('min_score is NaN')
        self.capacity = int(capacity)
        if not 1 <= self.capacity <= MAX_DETECTIONS:
            raise ValueError('capacity must lie in [1, 2^24], got %d' % self.capacity)
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('the evaluator runs on the GPU (no CPU fallback)')
        self.lib = _lib.load()
        T, C, A, Mx, R, dev = len(self._thresholds), self._num_classes, len(self._areas), len(self._max_dets), len(self._rec), self.device
        self._thr = (ctypes.c_float * T)(*self._thresholds)
        self._area_arr = (ctypes.c_float * (2 * A))(*[v for r in self._areas for v in r])
        self._md = (ctypes.c_int * Mx)(*self._max_dets)
        self._rec_dev = torch.from_numpy(self._rec).to(dev)
        cap = self.capacity
        if storage is not None:
            sizes = (cap, cap, cap * A, cap)
            for b, dt, sz in zip(storage, (torch.float32, torch.int32, torch.int32, torch.int32), sizes):
                if b.device != dev or b.dtype != dt or b.dim() != 1 or not b.is_contiguous() or b.numel() < sz:
                    raise ValueError('storage: contiguous 1-d float32 / int32 / int32 [capacity * A] / int32 GPU tensors of at least the capacity')
            self._bufs = tuple(b[:sz] for b, sz in zip(storage, sizes))
        else:
            self._bufs = (torch.empty(cap, dtype=torch.float32, device=dev), torch.empty(cap, dtype=torch.int32, device=dev),
                          torch.empty(cap * A, dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.int32, device=dev))
        self._ws = torch.empty(self.lib.effdet_coco_sorted_workspace_bytes(cap, C, A) // 8, dtype=torch.int64, device=dev)
        self._result = torch.zeros(self.lib.effdet_coco_sorted_result_bytes(T, C, A, Mx) // 8, dtype=torch.int64, device=dev)
        self._precision = torch.zeros(T, R, C, A, Mx, dtype=torch.float64, device=dev) if keep_precision else None
        self._state = torch.zeros(4, dtype=torch.int32, device=dev)          # cursor, lost, NaN scores, 0
        self._npig = torch.zeros(C * A, dtype=torch.int32, device=dev)
        self._last_rank = None                                                # [B, max_det] int32 of the last add_batch (test accessor)

    def _st(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def clear(self):
        """Forget everything (cursor and counters are reset on the device, no synchronisation)."""
        self._state.zero_()
        self._npig.zero_()

    def add_batch(self, det, count, gt_boxes, gt_cls, gt_crowd=None, gt_area=None):
        """det [B, max_det, 6] rows x1,y1,x2,y2,score,class (1-based) in descending score order, `count[b]` valid rows; gt_boxes
        [B, M, 4] yxyx, gt_cls [B, M] 1-based (<= 0: padding), gt_crowd [B, M] bool or None, gt_area [B, M] float32 or None (the
        box area).  -> flag words [B, max_det, A] int32: bit t = true positive at threshold t, bit 16 + t = ignored there, bit 31
        (negative) = dropped."""
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
            gt_crowd, gt_area, M = None, None, 1
        if gt_crowd is not None:
            gt_crowd = gt_crowd.to(device=dev, dtype=torch.uint8).contiguous()
            if tuple(gt_crowd.shape) != (B, M):
                raise ValueError('gt_crowd must be [B, M]')
        if gt_area is not None:
            gt_area = gt_area.to(device=dev, dtype=torch.float32).contiguous()
            if tuple(gt_area.shape) != (B, M):
                raise ValueError('gt_area must be [B, M]')
        A = len(self._areas)
        flags = torch.empty(B, max_det, A, dtype=torch.int32, device=dev)
        rank = torch.empty(B, max_det, dtype=torch.int32, device=dev)
        kept = torch.empty(2 * B, dtype=torch.int32, device=dev)
        st = self._st()
        _lib.check(self.lib.effdet_coco_match(st, det.data_ptr(), count.data_ptr(), gt_boxes.data_ptr(), gt_cls.data_ptr(),
                                              gt_crowd.data_ptr() if gt_crowd is not None else None,
                                              gt_area.data_ptr() if gt_area is not None else None, B, max_det, M, self._num_classes,
                                              self._thr, len(self._thresholds), self._area_arr, A, self._max_dets[-1], self.min_score,
                                              flags.data_ptr(), rank.data_ptr(), kept.data_ptr(), self._npig.data_ptr()),
                   'effdet_coco_match')
        _lib.check(self.lib.effdet_coco_append(st, det.data_ptr(), flags.data_ptr(), rank.data_ptr(), kept.data_ptr(), B, max_det, A,
                                               self._bufs[0].data_ptr(), self._bufs[1].data_ptr(), self._bufs[2].data_ptr(),
                                               self._bufs[3].data_ptr(), self.capacity, self._state.data_ptr()), 'effdet_coco_append')
        self._last_rank = rank
        return flags

    def enqueue(self):
        """Sort + AP / AR into the result block on the device; no host synchronisation."""
        _lib.check(self.lib.effdet_coco_sorted(self._st(), self._bufs[0].data_ptr(), self._bufs[1].data_ptr(), self._bufs[2].data_ptr(),
                                               self._bufs[3].data_ptr(), self.capacity, -1, self._state.data_ptr(), len(self._thresholds),
                                               self._num_classes, len(self._areas), self._md, len(self._max_dets),
                                               self._rec_dev.data_ptr(), len(self._rec), self._npig.data_ptr(), self._ws.data_ptr(),
                                               self._ws.numel() * 8, self._result.data_ptr(),
                                               self._precision.data_ptr() if self._precision is not None else None),
                   'effdet_coco_sorted')

    def result(self):
        """The result block of the last `enqueue()` (ONE device-to-host copy) -> dict(n, lost, nan_scores, ap / ar [T, C, A, Mx]
        float64 (NaN where the class has no box that counts in the area range), npig [C, A], block: the raw int64 words)."""
        block = self._result.cpu()
        r = parse_coco_result(block)
        if r['lost']:
            raise RuntimeError('%d detections were lost: more were added than the capacity of %d holds' % (r['lost'], self.capacity))
        r['block'] = block.numpy()
        return r

    def precision(self):
        """After `enqueue()` with keep_precision: the table [T, R, C, A, Mx] float64 on the device (NaN where npig = 0)."""
        if self._precision is None:
            raise RuntimeError('constructed without keep_precision=True')
        return self._precision

    def sorted(self):
        """After `enqueue()`: (class [n] int64, score [n] float32, flag words [n, A] uint32, rank [n] int32, entry index [n]) in
        the sorted order (debug / test accessor; synchronises)."""
        C, A = self._num_classes, len(self._areas)
        ws = self._ws.view(torch.uint8)
        off = [self.lib.effdet_coco_sorted_offset(self.capacity, C, A, w) for w in range(4)]
        n = min(int(self._state[0].item()), self.capacity)
        get = lambda o, nbytes, dt: ws[o:o + nbytes].cpu().numpy().view(dt)
        keys, index = get(off[0], 8 * n, np.uint64), get(off[1], 4 * n, np.uint32)
        words, ranks = get(off[2], 4 * n * A, np.uint32).reshape(n, A), get(off[3], 4 * n, np.int32)
        cls = (keys >> np.uint64(32)).astype(np.int64)
        k = ~(keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)                 # the order-preserving map of the float32 bits
        bits = np.where(k & np.uint32(0x80000000), k ^ np.uint32(0x80000000), ~k)
        valid = cls < C
        return cls[valid], bits.view(np.float32)[valid], words[valid], ranks[valid], index[valid]

    # ---- host glue: COCOeval.summarize ----------------------------------------------------------------------------------------
    def _mean(self, x, thr, area, m):
        if area not in self._area_labels:
            return -1.0
        s = x[:, :, self._area_labels.index(area), m]
        if thr is not None:
            s = s[[t for t, v in enumerate(self._thresholds) if abs(v - thr) < 1e-6]]
        s = s[~np.isnan(s)]
        return float(np.mean(s)) if s.size else -1.0

    def evaluate(self):
        """`enqueue()` + `result()` -> dict with the twelve COCO figures under pycocotools' wording, 'AP/<name>' per class
        (area 'all', the largest max_dets, NaN without ground truth) and 'stats': the length-12 array in COCOeval.stats order
        (-1 where no cell takes part, as pycocotools prints it)."""
        self.enqueue()
        r = self.result()
        ap, ar = r['ap'], r['ar']
        iou = '%.2f:%.2f' % (self._thresholds[0], self._thresholds[-1])
        last = len(self._max_dets) - 1
        rows = [('AP', iou, None, 'all', last), ('AP', '0.50', 0.5, 'all', last), ('AP', '0.75', 0.75, 'all', last),
                ('AP', iou, None, 'small', last), ('AP', iou, None, 'medium', last), ('AP', iou, None, 'large', last),
                ('AR', iou, None, 'all', 0), ('AR', iou, None, 'all', min(1, last)), ('AR', iou, None, 'all', last),
                ('AR', iou, None, 'small', last), ('AR', iou, None, 'medium', last), ('AR', iou, None, 'large', last)]
        out, stats = {}, []
        for kind, label, thr, area, m in rows:
            v = self._mean(ap if kind == 'AP' else ar, thr, area, m)
            stats.append(v)
            out['%s@[IoU=%s|area=%s|maxDets=%d]' % (kind, label, area, self._max_dets[m])] = v
        names = {cat['id']: cat['name'] for cat in self._categories}
        a_all = self._area_labels.index('all') if 'all' in self._area_labels else 0
        for c in range(self._num_classes):
            v = ap[:, c, a_all, last]
            v = v[~np.isnan(v)]
            out['AP/%s' % names.get(c + 1, str(c + 1))] = float(np.mean(v)) if v.size else float('nan')
        out['stats'] = np.array(stats)
        self.stats = out['stats']
        return out
