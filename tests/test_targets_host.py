"""oracle/targets.py against the reference's TargetAssigner fixtures (no GPU): first half of the usual two steps - the oracle
is pinned to the reference here, the device is compared with the oracle in tests/test_targets_gpu.py.

Matches, class targets and num_positives are compared exactly; box targets bit for bit in float32 (the reference's and the
oracle's logarithm are the same torch CPU operation on bit-identical quotients)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import targets as ot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE_TAGS = 'abcdefghi'


def _anchors128():
    from ood_object_detection_amd.effdet.anchors import Anchors
    return Anchors(3, 7, 3, [(1.0, 1.0), (1.4, 0.7), (0.7, 1.4)], 4.0, (128, 128)).boxes


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def test_oracle_assign_reproduces_labeler_fixture(golden):
    g = golden('labeler')
    A = _anchors128()
    for i in range(4):
        boxes, cls = torch.from_numpy(g['gt_boxes%d' % i]), torch.from_numpy(g['gt_cls%d' % i])
        keep = cls > -1
        match, cls_t, box_t, npos = ot.assign(A, boxes[keep], cls[keep], 0.5)
        assert np.array_equal(match.numpy(), g['match%d' % i])
        assert np.array_equal(cls_t.numpy(), g['cls_flat%d' % i])
        assert npos == int(g['npos'][i])
        assert _same_bits(box_t.numpy(), g['box_flat%d' % i])


@pytest.mark.parametrize('fv', [1, 0])
@pytest.mark.parametrize('tag', list(EDGE_TAGS))
def test_oracle_assign_reproduces_edge_fixture(golden, tag, fv):
    g = golden('labeler_edges')
    assert ''.join(g['tags']) == EDGE_TAGS
    A = _anchors128()
    boxes, cls = torch.from_numpy(g['gt_boxes_' + tag]), torch.from_numpy(g['gt_cls_' + tag])
    keep = cls > -1 if fv else torch.ones_like(cls, dtype=torch.bool)
    key = '%s_fv%d' % (tag, fv)
    for chunk in (8192, 1000):                                       # chunk borders must not show
        match, cls_t, box_t, npos = ot.assign(A, boxes[keep], cls[keep], 0.5, chunk=chunk)
        assert np.array_equal(match.numpy(), g['match_' + key].astype(np.int64))
        assert np.array_equal(cls_t.numpy(), g['cls_' + key].astype(np.int64))
        assert npos == int(g['npos_' + key])
        assert _same_bits(box_t[match >= 0].numpy(), g['box_' + key])
        assert not bool(box_t[match < 0].any())


def test_edge_fixture_holds_the_cases_it_is_for(golden):
    """what the fixture says the REFERENCE did on each edge, so that a regenerated fixture cannot quietly lose one"""
    g = golden('labeler_edges')
    A = _anchors128()
    m = lambda key: g['match_' + key].astype(np.int64)
    # (a) identical boxes: the second row owns nothing
    assert (m('a_fv1') == 0).any() and not (m('a_fv1') == 1).any()
    # (b) one best anchor for two different rows: the lower row has it
    sim = ot.iou_yxyx(torch.from_numpy(g['gt_boxes_b']), A)
    k = int(sim[0].argmax())
    assert int(sim[1].argmax()) == k and not torch.equal(sim[0], sim[1]) and m('b_fv1')[k] == 0
    # (c) IoU 0 everywhere: forced onto anchor 0;  (d) zero-area rows likewise, the lowest such row wins
    assert float(ot.iou_yxyx(torch.from_numpy(g['gt_boxes_c'][1:]), A).max()) == 0.0 and m('c_fv1')[0] == 1
    assert m('d_fv1')[0] == 0 and not (m('d_fv1') == 1).any()
    # (e) IoU exactly 1
    assert float(ot.iou_yxyx(torch.from_numpy(g['gt_boxes_e'][:1]), A).max()) == 1.0
    # (f), (g) rows of class -1: invisible when filtered; kept otherwise, class target -2; (f) differs in anchor 0 alone
    assert m('f_fv0')[0] == 1 and g['cls_f_fv0'][0] == -2 and g['cls_f_fv1'][0] == -1
    assert int((g['cls_f_fv0'] != g['cls_f_fv1']).sum()) == 1 and int(g['npos_f_fv0']) == int(g['npos_f_fv1']) + 1
    t = g['box_f_fv0'][0]                                            # anchor 0 is the first matched anchor
    assert t[0] == t[1] == -0.125 and t[2] == t[3] and abs(float(t[2]) + 21.886) < 1e-3
    assert int((g['cls_g_fv0'] == -2).sum()) > 1 and not (g['cls_g_fv1'] == -2).any()
    # (h) 40 rows, tiny ones among them;  (i) nothing
    hb = g['gt_boxes_h']
    assert hb.shape[0] == 40 and ((hb[:, 2] - hb[:, 0]) <= 4).sum() >= 5
    assert g['gt_boxes_i'].shape[0] == 0 and int(g['npos_i_fv1']) == 0 and (m('i_fv1') == -1).all()
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'labeler_edges.npz')) < 100 * 1024


def test_oracle_relabel_reproduces_task_cls_fixture(golden):
    g = golden('labeler_task_cls')
    task = int(g['task_cls'])
    A = _anchors128()
    for i in range(int(g['n_images'])):
        boxes, cls = torch.from_numpy(g['gt_boxes%d' % i]).reshape(-1, 4), torch.from_numpy(g['gt_cls%d' % i])
        before = cls.clone()
        new = ot.relabel_task_cls(boxes, cls, task, 0.9)
        assert torch.equal(cls, before)
        assert np.array_equal(new.numpy(), g['relabelled%d' % i])
        keep = new > -1
        _, cls_t, box_t, npos = ot.assign(A, boxes[keep], new[keep], 0.5)
        assert np.array_equal(cls_t.numpy(), g['cls_flat%d' % i])
        assert npos == int(g['npos'][i])
        assert _same_bits(box_t.numpy(), g['box_flat%d' % i])


def test_float64_encode_is_the_float32_encode_up_to_the_logarithm():
    """dtype=float64: ty / tx are the float32 values; th / tw are the float64 log of the float32 quotient, which the float32 log
    (correct to 1 ulp in torch's CPU library as well) approximates"""
    A = _anchors128()
    rs = np.random.RandomState(5)
    y0, x0 = rs.uniform(0, 90, 30), rs.uniform(0, 90, 30)
    boxes = torch.from_numpy(np.stack([y0, x0, y0 + rs.uniform(2, 60, 30), x0 + rs.uniform(2, 60, 30)], 1).astype(np.float32))
    cls = torch.from_numpy(rs.randint(1, 7, 30))
    m32, c32, b32, n32 = ot.assign(A, boxes, cls, 0.5)
    m64, c64, b64, n64 = ot.assign(A, boxes, cls, 0.5, dtype=torch.float64)
    assert torch.equal(m32, m64) and torch.equal(c32, c64) and n32 == n64 and b64.dtype == torch.float64
    assert torch.equal(b32[:, :2].double(), b64[:, :2])
    ulp = np.spacing(np.maximum(np.abs(b64[:, 2:].numpy()), 1.0).astype(np.float32)).astype(np.float64)
    assert (np.abs(b32[:, 2:].double().numpy() - b64[:, 2:].numpy()) <= 2 * ulp).all()


def test_first_maximum_and_lowest_row_rules():
    """the tie rules, on a problem small enough to read: integer boxes, IoU exactly 0.5"""
    A = torch.tensor([[0, 0, 10, 10], [0, 20, 10, 30], [0, 40, 10, 50]], dtype=torch.float32)
    # row 0 has IoU 0.5 with anchors 0 and 1 (first one is forced); row 1 equals row 0 (owns nothing); row 2 is far away
    gt = torch.tensor([[0, 0, 10, 30], [0, 0, 10, 30], [100, 100, 110, 110]], dtype=torch.float32)
    sim = ot.iou_yxyx(gt, A)
    assert sim[0, 0] == sim[0, 1] > 0 and sim[0, 2] == 0 and float(sim[2].max()) == 0
    gt2 = torch.tensor([[0, 0, 10, 20], [0, 20, 10, 40]], dtype=torch.float32)
    assert ot.iou_yxyx(gt2, A)[0].tolist() == [0.5, 0.0, 0.0]
    match, cls_t, _, npos = ot.assign(A, gt2, torch.tensor([4, 2]), 0.5)
    assert match.tolist() == [0, 1, -1] and cls_t.tolist() == [3, 1, -1] and npos == 2       # 0.5 is matched, not background
    match, _, _, _ = ot.assign(A, gt, torch.tensor([1, 2, 3]), 0.5)
    assert match.tolist() == [0, -1, -1]          # rows 0, 1 and 2 (IoU 0 -> column 0) all claim anchor 0: row 0 has it
    assert ot.assign(A, gt[:0], torch.zeros(0, dtype=torch.int64), 0.5)[0].tolist() == [-1, -1, -1]


def test_rows_entry_point_declared_bound_and_exported():
    from ood_object_detection_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'effdet_hip.h')).read()
    assert re.search(r'\bint\s+effdet_label_anchors_rows\s*\(', header)
    assert _lib.SIGNATURES['effdet_label_anchors_rows'] == _lib.SIGNATURES['effdet_label_anchors']
    assert re.search(r'#define\s+EFFDET_LABEL_PAD\s+\(-0x7fffffffffffffffLL - 1\)', header) and _lib.LABEL_PAD == -2 ** 63
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), 'effdet_label_anchors_rows')
