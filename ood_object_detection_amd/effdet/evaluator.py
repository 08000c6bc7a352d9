"""`effdet.evaluator` (reference: effdet/evaluator.py): the validation metric behind `create_evaluator(name, dataset)`.

`CocoEvaluator` is COCO `bbox` mAP@[.5:.95] - what the reference gets from pycocotools' COCOeval through a json file - computed
on the device by `CocoDetectionEvaluator` (csrc/coco_eval.hip).  `PascalEvaluator` / `OpenImagesEvaluator` / `OpenImagesChallengeEvaluator`
run on the device evaluators of effdet/evaluation (group-of boxes: csrc/openimages_eval.hip).  The ground truth of the whole dataset is uploaded once, as padded tables indexed by image index;
`add_predictions(detections, target)` gathers the batch's rows with `target['img_idx']` on the device, so a validation loop reads
nothing back before `evaluate()`.  Ground truth comes from `dataset.parser` as plain data (no pycocotools import):
`parser.img_ids`, `parser.coco.imgToAnns[img_id]` (dicts with `bbox` xywh, `category_id`, `iscrowd`, `area`), `parser.cat_ids`
and `parser.cat_id_to_label` when set.  Boxes are NOT filtered the way the training parser filters them: COCOeval sees every
annotation.  `save()` writes the COCO-style json from predictions kept on the host, only with `keep_predictions=True`.
`LvisEvaluator` is LVIS `bbox` AP under the federated rules (`LvisDetectionEvaluator`, csrc/lvis_eval.hip), from an LVIS json
dict through `lvis_ground_truth`; `create_evaluator` mirrors the reference's dispatch and does not name it.
"""
import abc
import json
import logging

import numpy as np
import torch
import torch.distributed as dist

from .distributed import all_gather_container
from .evaluation import (CocoDetectionEvaluator, LvisDetectionEvaluator, ObjectDetectionEvaluator, OpenImagesDetectionEvaluator,
                         PascalDetectionEvaluator)
from .evaluation import OpenImagesChallengeEvaluator as OpenImagesChallengeDetectionEvaluator
from .evaluation import CalibrationEvaluator as CalibrationDetectionEvaluator

_logger = logging.getLogger(__name__)

__all__ = ['CocoEvaluator', 'LvisEvaluator', 'PascalEvaluator', 'OpenImagesEvaluator', 'OpenImagesChallengeEvaluator', 'CalibrationEvaluator', 'create_evaluator',
           'coco_ground_truth', 'lvis_ground_truth']


def coco_ground_truth(anns, cat_id_to_label=None, cat_ids=None, M=None):
    """anns: per image a list of COCO annotation dicts (`bbox` x, y, w, h; `category_id`; optional `iscrowd`, `area`, `ignore`).
    -> (gt_boxes [B, M, 4] float32 yxyx, gt_cls [B, M] int64 1-based label (-1: padding), gt_crowd [B, M] uint8, gt_area [B, M]
    float32).  The label is cat_id_to_label[category_id] when the map is given, else the category id itself; an annotation whose
    category is not in the map (or not in cat_ids, when given) is left out, as COCOeval leaves out categories it was not asked
    for.  crowd = iscrowd or ignore (COCOeval._prepare); area = the annotation's `area`, w * h when it has none.  M: the padded
    length, at least the longest list (default: exactly that, and at least 1)."""
    known = set(cat_ids) if cat_ids is not None else None
    rows = []
    for per_image in anns:
        keep = []
        for a in per_image:
            cid = a['category_id']
            if known is not None and cid not in known:
                continue
            if cat_id_to_label:
                if cid not in cat_id_to_label:
                    continue
                label = int(cat_id_to_label[cid])
            else:
                label = int(cid)
            if label < 1:
                raise ValueError('labels are 1-based, got %d for category %r' % (label, cid))
            x, y, w, h = (float(v) for v in a['bbox'])
            crowd = 1 if (a.get('iscrowd', 0) or a.get('ignore', 0)) else 0
            keep.append(((y, x, y + h, x + w), label, crowd, float(a['area']) if 'area' in a else w * h))
        rows.append(keep)
    longest = max([len(r) for r in rows] + [1])
    if M is None:
        M = longest
    if M < longest:
        raise ValueError('M = %d is shorter than the longest annotation list (%d)' % (M, longest))
    B = len(rows)
    boxes, cls = np.zeros((B, M, 4), np.float32), np.full((B, M), -1, np.int64)
    crowd, area = np.zeros((B, M), np.uint8), np.zeros((B, M), np.float32)
    for i, r in enumerate(rows):
        for j, (b, label, cr, ar) in enumerate(r):
            boxes[i, j], cls[i, j], crowd[i, j], area[i, j] = b, label, cr, ar
    return torch.from_numpy(boxes), torch.from_numpy(cls), torch.from_numpy(crowd), torch.from_numpy(area)


def lvis_ground_truth(dataset_dict, cat_id_to_label=None, M=None, Kn=None, Ke=None):
    """dataset_dict: an LVIS annotation json as a dict - `images` (dicts with `id`, `neg_category_ids`,
    `not_exhaustive_category_ids`), `annotations` (dicts with `image_id`, `bbox` x, y, w, h, `area`, `category_id`), `categories`
    (dicts with `id`, `name`, `frequency`).  Pure host.  -> dict(gt_boxes [N, M, 4] float32 yxyx, gt_cls [N, M] int64 1-based label
    (-1: padding), gt_area [N, M] float32 (the annotation's `area`, w * h without one), neg_cls [N, Kn] and nel_cls [N, Ke] int64
    1-based labels (-1: padding), img_ids: row i = image i of `images`, categories: [{'id': label, 'name', 'frequency'}]).  The
    label is cat_id_to_label[category_id] when the map is given, else the category id itself; annotations and list entries of a
    category outside the map or outside `categories` are left out.  M, Kn, Ke: padded lengths, at least the longest list (default:
    exactly that, and at least 1)."""
    cats = dataset_dict['categories']
    known = {c['id'] for c in cats}

    def label(cid):
        if cid not in known or (cat_id_to_label and cid not in cat_id_to_label):
            return None
        lab = int(cat_id_to_label[cid]) if cat_id_to_label else int(cid)
        if lab < 1:
            raise ValueError('labels are 1-based, got %d for category %r' % (lab, cid))
        return lab
    categories = []
    for c in cats:
        if label(c['id']) is not None:
            entry = {'id': label(c['id']), 'name': str(c.get('name', c['id']))}
            if 'frequency' in c:
                entry['frequency'] = c['frequency']
            categories.append(entry)
    images = dataset_dict['images']
    row = {im['id']: i for i, im in enumerate(images)}
    boxes = [[] for _ in images]
    for a in dataset_dict['annotations']:
        lab = label(a['category_id'])
        if lab is None or a['image_id'] not in row:
            continue
        x, y, w, h = (float(v) for v in a['bbox'])
        boxes[row[a['image_id']]].append(((y, x, y + h, x + w), lab, float(a['area']) if 'area' in a else w * h))
    lists = [[[l for l in (label(c) for c in im.get(key, ())) if l is not None] for im in images]
             for key in ('neg_category_ids', 'not_exhaustive_category_ids')]

    def padded(name, asked, rows):
        longest = max([len(r) for r in rows] + [1])
        if asked is not None and asked < longest:
            raise ValueError('%s = %d is shorter than the longest list (%d)' % (name, asked, longest))
        return longest if asked is None else asked
    M, Kn, Ke = padded('M', M, boxes), padded('Kn', Kn, lists[0]), padded('Ke', Ke, lists[1])
    N = len(images)
    gt_boxes, gt_cls, gt_area = np.zeros((N, M, 4), np.float32), np.full((N, M), -1, np.int64), np.zeros((N, M), np.float32)
    neg, nel = np.full((N, Kn), -1, np.int64), np.full((N, Ke), -1, np.int64)
    for i in range(N):
        for j, (b, lab, ar) in enumerate(boxes[i]):
            gt_boxes[i, j], gt_cls[i, j], gt_area[i, j] = b, lab, ar
        neg[i, :len(lists[0][i])] = lists[0][i]
        nel[i, :len(lists[1][i])] = lists[1][i]
    return dict(gt_boxes=torch.from_numpy(gt_boxes), gt_cls=torch.from_numpy(gt_cls), gt_area=torch.from_numpy(gt_area),
                neg_cls=torch.from_numpy(neg), nel_cls=torch.from_numpy(nel), img_ids=[im['id'] for im in images], categories=categories)


class Evaluator:

    def __init__(self, distributed=False, pred_yxyx=False, keep_predictions=False, device='cuda:0'):
        self.distributed = distributed
        self.distributed_device = None
        self.pred_yxyx = pred_yxyx
        self.keep_predictions = keep_predictions
        self.device = torch.device(device)
        self.img_indices = []
        self.predictions = []
        self._tables = None                                                    # the dataset's ground truth on the device
        self._make, self._built = None, None                                   # the device evaluator is built at its first use

    @property
    def _evaluator(self):
        if self._built is None:
            self._built = self._make()
        return self._built

    def _ground_truth_tables(self):
        """-> tuple of [N, M, ...] tensors, row i = image index i"""
        raise NotImplementedError

    def _add(self, det, count, gt):
        raise NotImplementedError

    def add_predictions(self, detections, target):
        """detections [B, max_det, 6] (x1, y1, x2, y2 - or y1, x1, y2, x2 with pred_yxyx -, score, 1-based class; rows of zeros
        are padding), target['img_idx'] [B]: the images' indices in the dataset."""
        img_indices = target['img_idx']
        if self.distributed:
            if self.distributed_device is None:
                self.distributed_device = detections.device                    # cached to broadcast the metric later
            dist.barrier()
            detections = all_gather_container(detections)
            img_indices = all_gather_container(img_indices)
            if dist.get_rank() != 0:
                return
        if self._tables is None:
            self._tables = tuple(t.to(self.device) for t in self._ground_truth_tables())
        det = detections.to(self.device, torch.float32)
        if self.pred_yxyx:
            det = det[:, :, [1, 0, 3, 2, 4, 5]]
        idx = torch.as_tensor(img_indices).to(self.device, torch.int64)
        count = torch.full((det.shape[0],), det.shape[1], dtype=torch.int32, device=self.device)
        self._add(det, count, tuple(t[idx] for t in self._tables))
        if self.keep_predictions:                                              # the one host copy, only when asked
            self.img_indices.extend(int(i) for i in idx.cpu().tolist())
            self.predictions.extend(det.cpu().numpy())

    def _coco_predictions(self):
        coco_predictions, coco_ids = [], []
        for img_idx, img_dets in zip(self.img_indices, self.predictions):
            img_id = self._dataset.img_ids[img_idx]
            coco_ids.append(img_id)
            for det in img_dets:
                score = float(det[4])
                if score < .001:                                               # descending scores: stop below the threshold
                    break
                coco_predictions.append(dict(image_id=int(img_id), score=score, category_id=int(det[5]),
                                             bbox=[float(det[0]), float(det[1]), float(det[2] - det[0]), float(det[3] - det[1])]))
        return coco_predictions, coco_ids

    @abc.abstractmethod
    def evaluate(self):
        pass

    def _broadcast(self, metric):
        """rank 0's metric on every rank"""
        if not self.distributed:
            return metric
        t = torch.tensor(float(metric) if dist.get_rank() == 0 else 0.0, device=self.distributed_device, dtype=torch.float64)
        dist.broadcast(t, 0)
        return t.item()

    def save(self, result_file):
        """the kept predictions as a COCO-style result json"""
        if not self.keep_predictions:
            raise RuntimeError('save() needs keep_predictions=True: predictions stay on the device otherwise')
        if not self.distributed or dist.get_rank() == 0:
            assert len(self.predictions)
            coco_predictions, _ = self._coco_predictions()
            with open(result_file, 'w') as f:
                json.dump(coco_predictions, f, indent=4)


class CocoEvaluator(Evaluator):

    def __init__(self, dataset, distributed=False, pred_yxyx=False, keep_predictions=False, device='cuda:0', capacity=1 << 20):
        super().__init__(distributed=distributed, pred_yxyx=pred_yxyx, keep_predictions=keep_predictions, device=device)
        self._dataset = dataset.parser
        parser = self._dataset
        self._label_map = getattr(parser, 'cat_id_to_label', None) or None
        labels = sorted(self._label_map[c] for c in parser.cat_ids) if self._label_map else sorted(parser.cat_ids)
        if not labels:
            raise ValueError('the dataset has no categories')
        names = {(self._label_map[c] if self._label_map else c): c for c in parser.cat_ids}
        categories = [{'id': int(l), 'name': str(names[l])} for l in labels]
        self._make = lambda: CocoDetectionEvaluator(categories, min_score=0.001, capacity=capacity, device=device)

    def _ground_truth_tables(self):
        parser = self._dataset
        anns = [parser.coco.imgToAnns[img_id] for img_id in parser.img_ids]
        return coco_ground_truth(anns, cat_id_to_label=self._label_map, cat_ids=parser.cat_ids)

    def _add(self, det, count, gt):
        self._evaluator.add_batch(det, count, *gt)

    def reset(self):
        if self._built is not None:
            self._built.clear()
        self.img_indices = []
        self.predictions = []

    def evaluate(self):
        """COCO mAP@[.5:.95] (COCOeval.stats[0]); `self.metrics` keeps the whole dict.  Resets."""
        metric = 0.0
        if not self.distributed or dist.get_rank() == 0:
            self.metrics = self._evaluator.evaluate()
            for k, v in self.metrics.items():
                if k.startswith('A') and '@' in k:
                    _logger.info('%s = %.3f', k, v)
            metric = float(self.metrics['stats'][0])
        metric = self._broadcast(metric)
        self.reset()
        return metric


class LvisEvaluator(Evaluator):
    """LVIS `bbox` AP from an LVIS annotation dict (`lvis_ground_truth`): `target['img_idx']` indexes `dataset_dict['images']`."""

    def __init__(self, dataset_dict, distributed=False, pred_yxyx=False, keep_predictions=False, device='cuda:0', capacity=1 << 20,
                 cat_id_to_label=None, min_score=0.0):
        super().__init__(distributed=distributed, pred_yxyx=pred_yxyx, keep_predictions=keep_predictions, device=device)
        self._gt = lvis_ground_truth(dataset_dict, cat_id_to_label=cat_id_to_label)
        if not self._gt['categories']:
            raise ValueError('the dataset has no categories')
        self._dataset = type('Ids', (), dict(img_ids=self._gt['img_ids']))()
        self._make = lambda: LvisDetectionEvaluator(self._gt['categories'], min_score=min_score, capacity=capacity, device=device)

    def _ground_truth_tables(self):
        return tuple(self._gt[k] for k in ('gt_boxes', 'gt_cls', 'gt_area', 'neg_cls', 'nel_cls'))

    def _add(self, det, count, gt):
        self._evaluator.add_batch(det, count, *gt)

    def reset(self):
        if self._built is not None:
            self._built.clear()
        self.img_indices = []
        self.predictions = []

    def evaluate(self):
        """LVIS AP@[.5:.95] over all categories; `self.metrics` keeps the thirteen figures and the per-class AP.  Resets."""
        metric = 0.0
        if not self.distributed or dist.get_rank() == 0:
            self.metrics = self._evaluator.evaluate()
            for k, v in self.metrics.items():
                if k.startswith('A') and '/' not in k:
                    _logger.info('%s = %.3f', k, v)
            metric = float(self.metrics['AP'])
        metric = self._broadcast(metric)
        self.reset()
        return metric


class TfmEvaluator(Evaluator):
    """The TF-models protocol (PASCAL / OpenImages) on the device evaluators; ground truth from `parser.get_ann_info(i)`:
    dict(bbox [n, 4] yxyx, cls [n] 1-based)."""

    def __init__(self, dataset, distributed=False, pred_yxyx=False, evaluator_cls=ObjectDetectionEvaluator, keep_predictions=False,
                 device='cuda:0', **kw):
        super().__init__(distributed=distributed, pred_yxyx=pred_yxyx, keep_predictions=keep_predictions, device=device)
        self._dataset = dataset.parser
        self._make = lambda: evaluator_cls(categories=dataset.parser.cat_dicts, device=device, **kw)

    def _ground_truth_tables(self):
        parser = self._dataset
        gts = [parser.get_ann_info(i) for i in range(len(parser.img_ids))]
        for gt in gts:
            if any(np.asarray(gt[k]).any() for k in ('group_of', 'difficult') if k in gt):
                raise NotImplementedError('group-of / difficult ground truth is not built for this evaluator')
        M = max([len(np.asarray(gt['cls']).reshape(-1)) for gt in gts] + [1])
        boxes, cls = torch.zeros(len(gts), M, 4), torch.full((len(gts), M), -1, dtype=torch.int64)
        for i, gt in enumerate(gts):
            c = torch.as_tensor(np.asarray(gt['cls']), dtype=torch.int64).reshape(-1)
            boxes[i, :c.numel()] = torch.as_tensor(np.asarray(gt['bbox']), dtype=torch.float32).reshape(-1, 4)
            cls[i, :c.numel()] = c
        return boxes, cls

    def _add(self, det, count, gt):
        self._evaluator.add_batch(det, count, *gt)

    def reset(self):
        if self._built is not None:
            self._built.clear()
        self.img_indices = []
        self.predictions = []

    def evaluate(self):
        metric = 0.0
        if not self.distributed or dist.get_rank() == 0:
            self.metrics = self._evaluator.evaluate()
            _logger.info('Metrics:')
            for k, v in self.metrics.items():
                _logger.info(f'{k}: {v}')
            metric = float(self.metrics[self._evaluator._metric_names[0]])
        metric = self._broadcast(metric)
        self.reset()
        return metric


class PascalEvaluator(TfmEvaluator):

    def __init__(self, dataset, distributed=False, pred_yxyx=False, **kw):
        super().__init__(dataset, distributed=distributed, pred_yxyx=pred_yxyx, evaluator_cls=PascalDetectionEvaluator, **kw)


class OpenImagesEvaluator(TfmEvaluator):
    """OpenImages V2 on `OpenImagesDetectionEvaluator` (csrc/openimages_eval.hip): `parser.get_ann_info(i)` may carry `group_of` [n]
    bool beside bbox and cls; the flags are uploaded as a third table.  Without a group-of box the figures are the PASCAL
    protocol's.  `group_of_weight`, `iou_thresholds`, `capacity` and `evaluate_corlocs` go to the device evaluator; `difficult`
    ground truth still raises (the reference's OpenImages evaluators drop it)."""

    def __init__(self, dataset, distributed=False, pred_yxyx=False, evaluator_cls=OpenImagesDetectionEvaluator, **kw):
        kw.setdefault('metric_prefix', 'OpenImagesV2')
        super().__init__(dataset, distributed=distributed, pred_yxyx=pred_yxyx, evaluator_cls=evaluator_cls, **kw)

    def _annotations(self):
        parser = self._dataset
        gts = [parser.get_ann_info(i) for i in range(len(parser.img_ids))]
        for gt in gts:
            if 'difficult' in gt and np.asarray(gt['difficult']).any():
                raise NotImplementedError('difficult ground truth is not built for this evaluator')
        return gts

    def _ground_truth_tables(self):
        gts = self._annotations()
        M = max([len(np.asarray(gt['cls']).reshape(-1)) for gt in gts] + [1])
        boxes, cls = torch.zeros(len(gts), M, 4), torch.full((len(gts), M), -1, dtype=torch.int64)
        group_of = torch.zeros(len(gts), M, dtype=torch.uint8)
        for i, gt in enumerate(gts):
            c = torch.as_tensor(np.asarray(gt['cls']), dtype=torch.int64).reshape(-1)
            boxes[i, :c.numel()] = torch.as_tensor(np.asarray(gt['bbox']), dtype=torch.float32).reshape(-1, 4)
            cls[i, :c.numel()] = c
            if 'group_of' in gt and np.asarray(gt['group_of']).size:
                g = torch.as_tensor(np.asarray(gt['group_of']).astype(np.uint8)).reshape(-1)
                if g.numel() != c.numel():
                    raise ValueError('group_of: one flag per ground-truth box')
                group_of[i, :c.numel()] = g
        return boxes, cls, group_of

    def _add(self, det, count, gt):
        self._evaluator.add_batch(det, count, gt[0], gt[1], gt_group_of=gt[2])


class OpenImagesChallengeEvaluator(OpenImagesEvaluator):
    """The OpenImages Challenge metric: group-of boxes weigh 1 and the verified image-level labels of `parser.get_ann_info(i)`
    (`img_cls`, else `labeled_cls`: 1-based classes) decide, with the boxes' classes, which detections of an image are evaluated."""

    def __init__(self, dataset, distributed=False, pred_yxyx=False, **kw):
        kw.setdefault('metric_prefix', 'OpenImagesDetectionChallenge')
        super().__init__(dataset, distributed=distributed, pred_yxyx=pred_yxyx, evaluator_cls=OpenImagesChallengeDetectionEvaluator, **kw)

    def _ground_truth_tables(self):
        boxes, cls, group_of = super()._ground_truth_tables()
        lists = []
        for gt in self._annotations():
            l = gt['img_cls'] if 'img_cls' in gt else gt.get('labeled_cls', [])
            lists.append(torch.as_tensor(np.asarray(l), dtype=torch.int64).reshape(-1))
        K = max([l.numel() for l in lists] + [1])
        labels = torch.zeros(len(lists), K, dtype=torch.int64)
        for i, l in enumerate(lists):
            labels[i, :l.numel()] = l
        return boxes, cls, group_of, labels

    def _add(self, det, count, gt):
        self._evaluator.add_batch(det, count, gt[0], gt[1], gt_group_of=gt[2], labeled_cls=gt[3])


class CalibrationEvaluator(TfmEvaluator):
    """Calibration of the detection score on `effdet.evaluation.CalibrationEvaluator` (csrc/calibration_eval.hip): D-ECE, MCE, ACE,
    classwise ECE, LaECE, Brier and NLL under the PASCAL matching; `evaluate()` returns the D-ECE at the first threshold.
    `parser.get_ann_info(i)` may carry `difficult` [n] bool beside bbox and cls (matches with such boxes are ignored); `bins`,
    `score_threshold`, `iou_thresholds` and `capacity` go to the device evaluator."""

    def __init__(self, dataset, distributed=False, pred_yxyx=False, **kw):
        super().__init__(dataset, distributed=distributed, pred_yxyx=pred_yxyx, evaluator_cls=CalibrationDetectionEvaluator, **kw)

    @property
    def device_evaluator(self):
        """the `effdet.evaluation.CalibrationEvaluator` underneath (built at first use): what `DetectionCalibrator.fit` reads.
        `evaluate()` clears it, so a calibrator is fitted before `evaluate()` is called."""
        return self._evaluator

    def _ground_truth_tables(self):
        parser = self._dataset
        gts = [parser.get_ann_info(i) for i in range(len(parser.img_ids))]
        for gt in gts:
            if 'group_of' in gt and np.asarray(gt['group_of']).any():
                raise NotImplementedError('group-of ground truth is not built for this evaluator')
        M = max([len(np.asarray(gt['cls']).reshape(-1)) for gt in gts] + [1])
        boxes, cls = torch.zeros(len(gts), M, 4), torch.full((len(gts), M), -1, dtype=torch.int64)
        difficult = torch.zeros(len(gts), M, dtype=torch.uint8)
        for i, gt in enumerate(gts):
            c = torch.as_tensor(np.asarray(gt['cls']), dtype=torch.int64).reshape(-1)
            boxes[i, :c.numel()] = torch.as_tensor(np.asarray(gt['bbox']), dtype=torch.float32).reshape(-1, 4)
            cls[i, :c.numel()] = c
            if 'difficult' in gt and np.asarray(gt['difficult']).size:
                d = torch.as_tensor(np.asarray(gt['difficult']).astype(np.uint8)).reshape(-1)
                if d.numel() != c.numel():
                    raise ValueError('difficult: one flag per ground-truth box')
                difficult[i, :c.numel()] = d
        return boxes, cls, difficult

    def _add(self, det, count, gt):
        self._evaluator.add_batch(det, count, gt[0], gt[1], gt_difficult=gt[2])


def create_evaluator(name, dataset, distributed=False, pred_yxyx=False, **kw):
    if 'calibration' in name:
        return CalibrationEvaluator(dataset, distributed=distributed, pred_yxyx=pred_yxyx, **kw)
    elif 'coco' in name:
        return CocoEvaluator(dataset, distributed=distributed, pred_yxyx=pred_yxyx, **kw)
    elif 'openimages' in name:
        if 'challenge' in name:
            return OpenImagesChallengeEvaluator(dataset, distributed=distributed, pred_yxyx=pred_yxyx, **kw)
        return OpenImagesEvaluator(dataset, distributed=distributed, pred_yxyx=pred_yxyx, **kw)
    else:
        return PascalEvaluator(dataset, distributed=distributed, pred_yxyx=pred_yxyx, **kw)
