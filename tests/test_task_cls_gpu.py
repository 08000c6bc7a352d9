"""`AnchorLabeler.batch_label_anchors(..., task_cls=c)` (reference: effdet/anchors.py:396-403, used by dataloader.py:210 for
the projection images) on `effdet_relabel_task_cls`, against tests/golden/labeler_task_cls.npz - the reference's own
statements run by tools/make_golden.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
RATIOS = [(1.0, 1.0), (1.4, 0.7), (0.7, 1.4)]


def _labeler():
    from ood_object_detection_amd.effdet.anchors import Anchors, AnchorLabeler
    anchors = Anchors(3, 7, 3, RATIOS, 4.0, (128, 128)).to(DEV)
    return anchors, AnchorLabeler(anchors, num_classes=6, match_threshold=0.5)


def _inputs(g, dev):
    n = int(g['n_images'])
    boxes = [torch.from_numpy(g['gt_boxes%d' % i]).reshape(-1, 4).to(dev) for i in range(n)]
    cls = [torch.from_numpy(g['gt_cls%d' % i]).reshape(-1).to(dev) for i in range(n)]
    return n, boxes, cls


@pytest.mark.parametrize('where', ['cuda', 'cpu'])
def test_task_cls_relabelling_golden(golden, where):
    """Relabelled classes and class targets exact, box targets / num_positives as test_anchor_labeler_golden compares them;
    the caller's gt_classes tensors (on the GPU as dataloader.py passes them, or on the host) hold the new classes."""
    g = golden('labeler_task_cls')
    task_cls = int(g['task_cls'])
    anchors, lab = _labeler()
    n, gt_boxes, gt_cls = _inputs(g, DEV if where == 'cuda' else 'cpu')
    cls_l, box_l, npos = lab.batch_label_anchors(gt_boxes, gt_cls, filter_valid=True, task_cls=task_cls)
    for i in range(n):
        assert gt_cls[i].device.type == where and gt_cls[i].dtype == torch.int64
        assert np.array_equal(gt_cls[i].cpu().numpy(), g['relabelled%d' % i].reshape(-1)), (i, gt_cls[i])
    assert np.array_equal(npos.cpu().numpy(), g['npos'])
    cls_flat = torch.cat([c.reshape(n, -1) for c in cls_l], 1).cpu().numpy()
    box_flat = torch.cat([b.reshape(n, -1, 4) for b in box_l], 1).cpu().numpy()
    for i in range(n):
        assert np.array_equal(cls_flat[i], g['cls_flat%d' % i]), i
        assert np.abs(box_flat[i] - g['box_flat%d' % i]).max() <= 2e-6, i
    # the fixture really exercises the branch: some class changed, and the targets differ from the unrelabelled ones
    assert any(not np.array_equal(g['relabelled%d' % i], g['gt_cls%d' % i]) for i in range(n))
    _, gt_boxes0, gt_cls0 = _inputs(g, DEV)
    cls_plain, _, _ = lab.batch_label_anchors(gt_boxes0, gt_cls0)
    assert not np.array_equal(torch.cat([c.reshape(n, -1) for c in cls_plain], 1).cpu().numpy(), cls_flat)


def test_task_cls_none_is_the_plain_path_and_raw_entry_point(golden):
    """task_cls=None: the relabel launch is skipped - results bit-identical to the call without the argument, the caller's
    classes untouched.  Then the C entry point on padded tensors: padding rows stay -1, an image without a task box and a
    task class that no image has leave everything alone, bad arguments are refused."""
    from ood_object_detection_amd import _lib
    import _hip
    g = golden('labeler_task_cls')
    anchors, lab = _labeler()
    n, gt_boxes, gt_cls = _inputs(g, DEV)
    keep = [c.clone() for c in gt_cls]
    a = lab.batch_label_anchors(gt_boxes, gt_cls, filter_valid=True, task_cls=None)
    b = lab.batch_label_anchors(gt_boxes, gt_cls)
    for x, y in zip(a[0] + a[1] + [a[2]], b[0] + b[1] + [b[2]]):
        assert torch.equal(x, y)
    for c, k in zip(gt_cls, keep):
        assert torch.equal(c, k)

    lib = _lib.load()
    task_cls = int(g['task_cls'])
    Mmax = max(int(c.numel()) for c in gt_cls) + 2
    gb = torch.zeros(n, Mmax, 4, device=DEV)
    gc = torch.full((n, Mmax), -1, dtype=torch.int64, device=DEV)
    for i in range(n):
        m = gt_cls[i].numel()
        if m:
            gb[i, :m], gc[i, :m] = gt_boxes[i], gt_cls[i]
    before = gc.clone()
    assert lib.effdet_relabel_task_cls(_hip.stream(DEV), gb.data_ptr(), gc.data_ptr(), n, Mmax, task_cls, 0.9) == 0
    torch.cuda.synchronize()
    for i in range(n):
        m = gt_cls[i].numel()
        assert np.array_equal(gc[i, :m].cpu().numpy(), g['relabelled%d' % i].reshape(-1))
        assert bool((gc[i, m:] == -1).all())
    gc2 = before.clone()
    assert lib.effdet_relabel_task_cls(_hip.stream(DEV), gb.data_ptr(), gc2.data_ptr(), n, Mmax, 77, 0.9) == 0
    torch.cuda.synchronize()
    assert torch.equal(gc2, before)
    assert lib.effdet_relabel_task_cls(_hip.stream(DEV), gb.data_ptr(), gc2.data_ptr(), n, 513, task_cls, 0.9) != 0
    assert lib.effdet_relabel_task_cls(_hip.stream(DEV), None, gc2.data_ptr(), n, Mmax, task_cls, 0.9) != 0
    assert lib.effdet_relabel_task_cls(_hip.stream(DEV), gb.data_ptr(), gc2.data_ptr(), n, Mmax, -1, 0.9) != 0
