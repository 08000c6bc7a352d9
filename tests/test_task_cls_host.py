"""Host-side checks of the task_cls relabelling (no GPU): the new entry point is declared, bound and exported, and the fixture
tests/golden/labeler_task_cls.npz is self-consistent - its relabelled classes follow from its inputs by the rule of
effdet/anchors.py:396-403, with no IoU close enough to 0.9 for float32 rounding to decide a case."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_relabel_entry_point_declared_bound_and_exported():
    from ood_object_detection_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'effdet_hip.h')).read()
    assert re.search(r'\bint\s+effdet_relabel_task_cls\s*\(', header)
    restype, argtypes = _lib.SIGNATURES['effdet_relabel_task_cls']
    assert restype is ctypes.c_int and len(argtypes) == 7
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    import torch  # noqa: F401  (share torch's HIP runtime, see _lib.load)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), 'effdet_relabel_task_cls')


def _iou(a, b):
    """region_similarity_calculator.py:24-73 in float32: a [n,4], b [m,4] yxyx -> [n,m]"""
    f = np.float32
    ih = np.maximum(np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0]), f(0))
    iw = np.maximum(np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1]), f(0))
    inter = ih * iw
    area = lambda x: (x[:, 2] - x[:, 0]) * (x[:, 3] - x[:, 1])
    union = area(a)[:, None] + area(b)[None, :] - inter
    return np.where(inter == 0, f(0), inter / np.where(inter == 0, f(1), union))


def test_task_cls_fixture_is_consistent_and_covers_the_cases(golden):
    g = golden('labeler_task_cls')
    c = int(g['task_cls'])
    n = int(g['n_images'])
    seen = set()
    for i in range(n):
        boxes, cls, new = g['gt_boxes%d' % i].reshape(-1, 4), g['gt_cls%d' % i].reshape(-1), g['relabelled%d' % i].reshape(-1)
        assert boxes.dtype == np.float32 and cls.dtype == np.int64
        if cls.size == 0:
            seen.add('empty')
            assert new.size == 0
            continue
        task = cls == c
        if task.all():
            seen.add('all task')
            assert np.array_equal(new, cls)
            continue
        sims = _iou(boxes[task], boxes)
        assert np.abs(sims - np.float32(0.9)).min() > 1e-4           # the strict comparison is never decided by rounding
        hit = (sims > 0.9).any(0)
        assert np.array_equal(new, np.where(hit, c, cls)), i
        others = ~task
        if (hit & others & (cls > -1)).any():
            seen.add('relabelled')
        if (others & ~hit & (sims.max(0) > 0.8)).any():
            seen.add('just below')
        if (hit & (cls == -1)).any():
            seen.add('-1 overlapping')
        if task.sum() == 1 and others.sum() >= 3 and not hit[others].any() and sims[:, others].max() == 0:
            seen.add('disjoint others')
        assert int(g['cls_flat%d' % i].max()) <= 5 and g['box_flat%d' % i].shape[1] == 4
    assert seen == {'empty', 'all task', 'relabelled', 'just below', '-1 overlapping', 'disjoint others'}, seen
    assert g['npos'].shape == (n,)
