"""ORACLE (test infrastructure only - never imported by the product path).

Plain torch-on-CPU restatement of the training target assignment the fork runs in its data loaders
(AnchorLabeler.batch_label_anchors, effdet/anchors.py:384-438), written from the description of the operation:

  effdet/object_detection/region_similarity_calculator.py:24-73  IoU in float32: intersection (clamped heights * widths),
                                                                 areas, union = area_a + area_b - inter, 0 where inter == 0
  effdet/object_detection/argmax_matcher.py:116-146              per column (anchor) the row (box) with the largest IoU, the
                                                                 first one on ties; unmatched (-1) where threshold > max;
                                                                 force_match_for_each_row: every row claims the column of
                                                                 its largest IoU (first one on ties), and where several
                                                                 rows claim one column the lowest row gets it
  effdet/object_detection/target_assigner.py:146-220             class target = label of the matched row, box target =
                                                                 encode(matched box, anchor), zeros where unmatched
  effdet/object_detection/box_coder.py:81-110                    FasterRcnnBoxCoder.encode with eps 1e-8, no scale factors
  effdet/anchors.py:396-403, :416, :434                          task_cls relabelling, `cls - 1`, num_positives

Every float32 operation here is a separate, correctly rounded IEEE operation (subtract, multiply, add, divide, min, max), as
it is in the reference and in train_ops.hip (compiled with -ffp-contract=off), so IoU values and every decision taken on
them are bit-identical on all three sides.  Ties are resolved by explicit "lowest index" expressions, not by whatever
torch.max happens to return.  The only operation that is not correctly rounded is the logarithm of the box encode; see
`assign(..., dtype=torch.float64)`.

Pinned: tests/golden/labeler.npz, labeler_edges.npz and labeler_task_cls.npz were produced by the reference's own
TargetAssigner (tools/make_golden.py); tests/test_targets_host.py compares this file with them exactly.
"""
import torch

_EPS = 1e-8


def iou_yxyx(a, b):
    """a [M,4], b [N,4] yxyx -> [M,N] float32"""
    a, b = a.to(torch.float32), b.to(torch.float32)
    ih = (torch.minimum(a[:, 2:3], b[:, 2][None]) - torch.maximum(a[:, 0:1], b[:, 0][None])).clamp(min=0)
    iw = (torch.minimum(a[:, 3:4], b[:, 3][None]) - torch.maximum(a[:, 1:2], b[:, 1][None])).clamp(min=0)
    inter = ih * iw
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    union = area_a[:, None] + area_b[None] - inter
    return torch.where(inter == 0.0, torch.zeros_like(inter), inter / union)


def _first_where_max(x, dim):
    """(max along dim, lowest index that attains it)"""
    v = x.max(dim).values
    n = x.shape[dim]
    idx = torch.arange(n).reshape([n if d == dim else 1 for d in range(x.dim())])
    first = torch.where(x == v.unsqueeze(dim), idx, torch.full_like(idx, n)).min(dim).values
    return v, first


def match_anchors(anchors, gt_boxes, thr, chunk=8192):
    """-> match [N] int64: the row every anchor is assigned to, -1 = unmatched.  Anchors are processed `chunk` at a time, so
    the largest problem the kernel takes (196 416 anchors x 512 rows) holds a few tens of MB at once."""
    N, M = anchors.shape[0], gt_boxes.shape[0]
    match = torch.full((N,), -1, dtype=torch.int64)
    if M == 0:
        return match
    thr = torch.tensor(thr, dtype=torch.float32)                              # the kernel's threshold is a float
    row_best = torch.full((M,), -1.0, dtype=torch.float32)
    row_col = torch.zeros(M, dtype=torch.int64)
    for off in range(0, N, chunk):
        sim = iou_yxyx(gt_boxes, anchors[off:off + chunk])                    # [M, n]
        v, m = _first_where_max(sim, 0)
        match[off:off + chunk] = torch.where(thr > v, torch.full_like(m, -1), m)
        rv, rc = _first_where_max(sim, 1)
        better = rv > row_best                                                # strict: an earlier chunk keeps a tie
        row_best = torch.where(better, rv, row_best)
        row_col = torch.where(better, rc + off, row_col)
    for m in range(M - 1, -1, -1):                                            # descending: the lowest row is written last
        match[row_col[m]] = m
    return match


def encode_boxes(boxes, anchors, dtype=torch.float32):
    """FasterRcnnBoxCoder.encode -> [n,4] (ty, tx, th, tw) in `dtype`.

    float32: the reference's own operations, one by one.
    float64: ty / tx are the float32 values (only correctly rounded operations: nothing to gain), th / tw are the float64
             logarithm of the float32 quotient h / ha, w / wa - the exact value a float32 logf is an approximation of."""
    b, a = boxes.to(torch.float32), anchors.to(torch.float32)
    eps = torch.tensor(_EPS, dtype=torch.float32)
    ha0, wa0 = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
    yca, xca = a[:, 0] + ha0 / 2.0, a[:, 1] + wa0 / 2.0
    h0, w0 = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    yc, xc = b[:, 0] + h0 / 2.0, b[:, 1] + w0 / 2.0
    ha, wa, h, w = ha0 + eps, wa0 + eps, h0 + eps, w0 + eps
    tx, ty = (xc - xca) / wa, (yc - yca) / ha
    qw, qh = w / wa, h / ha
    tw, th = torch.log(qw.to(dtype)), torch.log(qh.to(dtype))
    return torch.stack([ty.to(dtype), tx.to(dtype), th, tw], 1)


def assign(anchors, gt_boxes, gt_labels, thr=0.5, dtype=torch.float32, chunk=8192):
    """anchors [N,4], gt_boxes [M,4] yxyx, gt_labels [M] (1-based classes; every row given takes part)
    -> match [N] int64, cls_t [N] int64 (label - 1, background -1), box_t [N,4] `dtype`, num_positives (int)"""
    anchors = anchors.to(torch.float32).reshape(-1, 4)
    gt_boxes = gt_boxes.to(torch.float32).reshape(-1, 4)
    gt_labels = gt_labels.to(torch.int64).reshape(-1)
    N = anchors.shape[0]
    match = match_anchors(anchors, gt_boxes, thr, chunk)
    pos = match >= 0
    cls_t = torch.full((N,), -1, dtype=torch.int64)
    box_t = torch.zeros(N, 4, dtype=dtype)
    if bool(pos.any()):
        cls_t[pos] = gt_labels[match[pos]] - 1
        box_t[pos] = encode_boxes(gt_boxes[match[pos]], anchors[pos], dtype)
    return match, cls_t, box_t, int(pos.sum())


def relabel_task_cls(gt_boxes, gt_cls, task_cls, thr=0.9):
    """anchors.py:396-403 on one image: every row whose IoU with some row of class task_cls is > thr takes that class.  The
    mask of task rows is built from the classes as given (a row that has just been relabelled does not relabel others).  An
    image without a row of class task_cls comes back unchanged.  -> new classes [M] int64 (the input is not modified)"""
    gt_boxes = gt_boxes.to(torch.float32).reshape(-1, 4)
    out = gt_cls.to(torch.int64).reshape(-1).clone()
    task = out == task_cls
    if bool(task.any()) and bool((~task).any()):
        over = (iou_yxyx(gt_boxes[task], gt_boxes) > torch.tensor(thr, dtype=torch.float32)).any(0)
        out[over] = task_cls
    return out
