"""effdet_label_anchors / effdet_label_anchors_rows / effdet_relabel_task_cls against oracle/targets.py (-m gpu), beyond the
reference fixtures: real anchor counts, Mmax up to 512, interleaved padding, ties, IoU exactly at the threshold, many rows on
one column, degenerate boxes, workspace handling.  oracle/targets.py itself is pinned to the reference's TargetAssigner in
tests/test_targets_host.py.

What is compared, and how (see oracle/targets.py): IoU is made of correctly rounded float32 operations on both sides, so
`match`, `cls_t`, `num_positives` and the box targets ty / tx are compared EXACTLY, with no excluded cases.  th / tw go
through logf: the device value is compared with the float64 logarithm of the float32 quotient and may differ by 2 float32
ulps at max(|ref|, 1) - OCML documents 1 ulp for logf, plus the final rounding of the reference value.

Largest th / tw deviation observed on an MI355X over this whole file: 1.80 float32 ulps (test_log_deviation_report prints
it on every run)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import targets as ot

DEV = 'cuda:0'
RATIOS = [(1.0, 1.0), (1.4, 0.7), (0.7, 1.4)]
PAD = -2 ** 63
_worst_log_ulps = [0.0]


def _std_anchors(size):
    from ood_object_detection_amd.effdet.anchors import Anchors
    return Anchors(3, 7, 3, RATIOS, 4.0, (size, size)).boxes


class Buffers(object):
    """device outputs + workspace of one (B, Mmax, N), reusable across calls"""

    def __init__(self, B, Mmax, N):
        from ood_object_detection_amd import _lib
        self.lib = _lib.load()
        self.B, self.Mmax, self.N = B, Mmax, N
        self.cls_t = torch.full((B, N), 77, dtype=torch.int64, device=DEV)
        self.box_t = torch.full((B, N, 4), 7.0, device=DEV)
        self.npos = torch.full((B,), 7.0, device=DEV)
        self.match = torch.full((B, N), 77, dtype=torch.int64, device=DEV)
        self.nbytes = self.lib.effdet_label_anchors_workspace_bytes(B, Mmax, N)
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device=DEV)


def _label(anchors, gb, gc, thr=0.5, rows=False, bufs=None, nbytes=None):
    """raw C-ABI call -> (rc, match, cls_t, box_t, npos) on the host"""
    import _hip
    gb, gc = torch.as_tensor(gb, dtype=torch.float32), torch.as_tensor(gc, dtype=torch.int64)
    B, Mmax = gc.shape
    N = anchors.shape[0]
    bufs = bufs or Buffers(B, Mmax, N)
    a = anchors.to(DEV).float().contiguous()
    gbd, gcd = gb.to(DEV).contiguous(), gc.to(DEV).contiguous()
    fn = bufs.lib.effdet_label_anchors_rows if rows else bufs.lib.effdet_label_anchors
    rc = fn(_hip.stream(DEV), a.data_ptr(), gbd.data_ptr() if Mmax else None, gcd.data_ptr() if Mmax else None, B, Mmax, N, thr,
            bufs.cls_t.data_ptr(), bufs.box_t.data_ptr(), bufs.npos.data_ptr(), bufs.match.data_ptr(), bufs.ws.data_ptr(),
            bufs.nbytes if nbytes is None else nbytes)
    torch.cuda.synchronize()
    return rc, bufs.match.cpu(), bufs.cls_t.cpu(), bufs.box_t.cpu(), bufs.npos.cpu()


def _check_boxes(got, ref64):
    """got [n,4] float32 from the device, ref64 [n,4] = oracle assign(dtype=float64); the rules of the module docstring"""
    got, ref64 = got.numpy(), ref64.numpy()
    assert np.array_equal(got[:, :2].astype(np.float64), ref64[:, :2], equal_nan=True), 'ty / tx differ'
    g, r = got[:, 2:].astype(np.float64), ref64[:, 2:]
    assert np.array_equal(np.isnan(g), np.isnan(r)) and np.array_equal(np.isinf(g), np.isinf(r))
    fin = np.isfinite(r)
    if fin.any():
        ulp = np.spacing(np.maximum(np.abs(r[fin]), 1.0).astype(np.float32)).astype(np.float64)
        dev = np.abs(g[fin] - r[fin]) / ulp
        _worst_log_ulps[0] = max(_worst_log_ulps[0], float(dev.max()))
        assert float(dev.max()) <= 2.0, 'th / tw off by %.3f float32 ulps' % float(dev.max())


def _check_against_oracle(anchors, gb, gc, out, thr=0.5, rows=False):
    rc, match, cls_t, box_t, npos = out
    assert rc == 0
    gb, gc = torch.as_tensor(gb, dtype=torch.float32), torch.as_tensor(gc, dtype=torch.int64)
    for b in range(gc.shape[0]):
        keep = gc[b] != PAD if rows else gc[b] > -1
        m, c, bt, n = ot.assign(anchors, gb[b][keep], gc[b][keep], thr, dtype=torch.float64)
        assert torch.equal(match[b], m), 'match differs in image %d at anchors %s' % (b, (match[b] != m).nonzero().flatten()[:8].tolist())
        assert torch.equal(cls_t[b], c)
        assert float(npos[b]) == n
        _check_boxes(box_t[b], bt)
    return match


# ------------------------------------------------------------------------------------------------ edge fixture
@pytest.mark.parametrize('filter_valid', [True, False])
def test_anchor_labeler_edge_fixture(golden, filter_valid):
    """tests/golden/labeler_edges.npz (the reference's TargetAssigner on ties, a shared best anchor, IoU 0 and 1, zero-area
    boxes, rows of class -1, 40 boxes, an empty image) through AnchorLabeler with both filter_valid settings, one batch.
    filter_valid=False keeps the rows of class -1: they are matched and give class target -2 (images f and g)."""
    from ood_object_detection_amd.effdet.anchors import Anchors, AnchorLabeler
    g = golden('labeler_edges')
    tags = [str(t) for t in g['tags']]
    fv = 1 if filter_valid else 0
    anchors = Anchors(3, 7, 3, RATIOS, 4.0, (128, 128)).to(DEV)
    A = anchors.boxes.cpu()
    lab = AnchorLabeler(anchors, num_classes=6, match_threshold=0.5)
    gt_boxes = [torch.from_numpy(g['gt_boxes_' + t]) for t in tags]
    gt_cls = [torch.from_numpy(g['gt_cls_' + t]) for t in tags]
    cls_l, box_l, npos = lab.batch_label_anchors(gt_boxes, [c.clone() for c in gt_cls], filter_valid=filter_valid)
    B = len(tags)
    cls_flat = torch.cat([c.reshape(B, -1) for c in cls_l], 1).cpu()
    box_flat = torch.cat([b.reshape(B, -1, 4) for b in box_l], 1).cpu()
    # the same through the C ABI, for the match vector: padded by hand like the wrapper does
    Mmax = max(int(c.shape[0]) for c in gt_cls)
    gb = torch.zeros(B, Mmax, 4)
    gc = torch.full((B, Mmax), -1 if filter_valid else PAD, dtype=torch.int64)
    for i in range(B):
        n = gt_cls[i].shape[0]
        gb[i, :n], gc[i, :n] = gt_boxes[i], gt_cls[i]
    rc, match, cls_raw, box_raw, npos_raw = _label(A, gb, gc, rows=not filter_valid)
    assert rc == 0
    for i, t in enumerate(tags):
        key = '%s_fv%d' % (t, fv)
        ref_match = torch.from_numpy(g['match_' + key].astype(np.int64))
        assert torch.equal(cls_flat[i], torch.from_numpy(g['cls_' + key].astype(np.int64))), t
        assert float(npos[i]) == float(g['npos_' + key]), t
        assert torch.equal(match[i], ref_match), t
        assert torch.equal(cls_raw[i], cls_flat[i]) and torch.equal(box_raw[i], box_flat[i]) and float(npos_raw[i]) == float(npos[i])
        pos = ref_match >= 0
        assert not bool(box_flat[i][~pos].any())
        # ty / tx: the fixture's bits; th / tw: 2 ulps around the float64 logarithm (the fixture holds the CPU's float32 log)
        ref = torch.from_numpy(g['box_' + key])
        assert torch.equal(box_flat[i][pos][:, :2], ref[:, :2]), t
        keep = gt_cls[i] > -1 if filter_valid else torch.ones_like(gt_cls[i], dtype=torch.bool)
        _check_boxes(box_flat[i][pos], ot.encode_boxes(gt_boxes[i][keep][ref_match[pos]], A[pos], torch.float64))
    if not filter_valid:
        f = tags.index('f')
        assert int(cls_flat[f, 0]) == -2 and int(match[f, 0]) == 1              # the loader's padding row, forced onto anchor 0


def test_anchor_labeler_task_cls_without_filter_keeps_negative_rows(golden):
    """task_cls together with filter_valid=False: relabelled classes as in the fixture, then every row takes part"""
    from ood_object_detection_amd.effdet.anchors import Anchors, AnchorLabeler
    g = golden('labeler_task_cls')
    task = int(g['task_cls'])
    anchors = Anchors(3, 7, 3, RATIOS, 4.0, (128, 128)).to(DEV)
    A = anchors.boxes.cpu()
    lab = AnchorLabeler(anchors, num_classes=6, match_threshold=0.5)
    n = int(g['n_images'])
    gt_boxes = [torch.from_numpy(g['gt_boxes%d' % i]).reshape(-1, 4) for i in range(n)]
    gt_cls = [torch.from_numpy(g['gt_cls%d' % i]).clone() for i in range(n)]
    given = [c.clone() for c in gt_cls]
    cls_l, box_l, npos = lab.batch_label_anchors(gt_boxes, gt_cls, filter_valid=False, task_cls=task)
    cls_flat = torch.cat([c.reshape(n, -1) for c in cls_l], 1).cpu()
    for i in range(n):
        new = ot.relabel_task_cls(gt_boxes[i], given[i], task)
        assert torch.equal(gt_cls[i], new) and np.array_equal(new.numpy(), g['relabelled%d' % i])     # caller's tensor rewritten
        m, c, bt, k = ot.assign(A, gt_boxes[i], new, 0.5)
        assert torch.equal(cls_flat[i], c) and float(npos[i]) == k


# ------------------------------------------------------------------------------------------------ real sizes
@pytest.mark.parametrize('Mmax', [1, 100, 512])
@pytest.mark.parametrize('B', [1, 8])
@pytest.mark.parametrize('size', [640, 768, 1024])
def test_label_anchors_real_sizes(size, B, Mmax):
    """standard anchors (76 725 / 110 484 / 196 416), box counts mixed from 0 to Mmax, padding rows between valid rows, rows
    of class -1 in the middle; the 640 px cases also run the `_rows` entry, where those rows take part"""
    from _seeded import label_case
    A = _std_anchors(size)
    assert A.shape[0] == {640: 76725, 768: 110484, 1024: 196416}[size]
    gb, gc = label_case(1000 + size + 10 * B + Mmax, B, Mmax, size)
    bufs = Buffers(B, Mmax, A.shape[0])
    _check_against_oracle(A, gb, gc, _label(A, gb, gc, bufs=bufs))
    if size == 640:
        gcr = np.where((gc == -1) & (gb[:, :, 2] == 0), PAD, gc)          # this generator's padding rows -> the entry's sentinel
        match = _check_against_oracle(A, gb, gcr, _label(A, gb, gcr, rows=True, bufs=bufs), rows=True)
        if Mmax == 512:
            assert bool((bufs.cls_t.cpu() == -2).any())                   # rows of class -1 are there and own anchors


def test_label_anchors_rejects_more_than_512_rows():
    from ood_object_detection_amd.effdet.anchors import Anchors, AnchorLabeler
    anchors = Anchors(3, 7, 3, RATIOS, 4.0, (128, 128)).to(DEV)
    A = anchors.boxes.cpu()
    gb = torch.zeros(1, 513, 4)
    gb[0, :, 2:] = 20.0
    gc = torch.ones(1, 513, dtype=torch.int64)
    for rows in (False, True):
        assert _label(A, gb, gc, rows=rows)[0] == -22
    lab = AnchorLabeler(anchors, num_classes=6)
    for fv in (True, False):
        with pytest.raises(RuntimeError):
            lab.batch_label_anchors([gb[0]], [gc[0]], filter_valid=fv)
    assert _label(A, gb[:, :512], gc[:, :512])[0] == 0


# ------------------------------------------------------------------------------------------------ synthetic anchors
def _strip(n):
    """n integer anchors [0, 10 i, 10, 10 i + 10]"""
    i = torch.arange(n, dtype=torch.float32) * 10
    return torch.stack([torch.zeros(n), i, torch.full((n,), 10.0), i + 10], 1)


def test_iou_exactly_at_the_threshold_is_matched():
    """[0,0,10,10] and [0,10,10,20] against the row [0,0,10,20]: IoU 100 / 200 = 0.5 exactly on both.  Anchor 0 is forced (first
    maximum of the row); anchor 1 is matched by the threshold alone, because unmatched is `threshold > max`: not background.
    With the threshold one float32 step above 0.5 it is background."""
    A = _strip(3)
    gb, gc = torch.tensor([[[0.0, 0, 10, 20]]]), torch.tensor([[4]])
    assert ot.iou_yxyx(gb[0], A)[0].tolist() == [0.5, 0.5, 0.0]
    out = _label(A, gb, gc, thr=0.5)
    assert out[1][0].tolist() == [0, 0, -1] and out[2][0].tolist() == [3, 3, -1] and float(out[4][0]) == 2
    _check_against_oracle(A, gb, gc, out, thr=0.5)
    up = float(np.nextafter(np.float32(0.5), np.float32(1)))
    out = _label(A, gb, gc, thr=up)
    assert out[1][0].tolist() == [0, -1, -1] and float(out[4][0]) == 1
    _check_against_oracle(A, gb, gc, out, thr=up)


@pytest.mark.parametrize('N', [1, 255, 256, 257])
def test_label_anchors_small_anchor_counts_full_of_ties(N):
    """integer anchors in a strip, rows that straddle two neighbouring anchors (IoU 0.5 with both: tie in the row) and
    overlap each other's anchors (tie in the column), around the workgroup size of 256"""
    rs = np.random.RandomState(N)
    A = _strip(N)
    M = 40
    gb = np.zeros((2, M, 4), np.float32)
    gc = np.full((2, M), -1, np.int64)
    for b in range(2):
        for m in range(0, M, 2 if b else 1):
            k = rs.randint(0, N)
            gb[b, m] = (0, 10 * k, 10, 10 * k + 20)
            gc[b, m] = rs.randint(1, 9)
    _check_against_oracle(A, gb, gc, _label(A, gb, gc))
    _check_against_oracle(A, gb, gc, _label(A, gb, gc, thr=0.75), thr=0.75)          # forced matches only


@pytest.mark.parametrize('where', ['workgroups', 'waves', 'lanes'])
def test_row_tie_between_anchors_takes_the_lowest_anchor(where):
    """one row with the same IoU (0.5) on several identical anchors that sit in different 256-anchor workgroups / different
    waves of one workgroup / one wave; at threshold 0.6 only the forced anchor is matched: the lowest index"""
    cols = {'workgroups': [700, 300, 5], 'waves': [200, 130, 70, 3], 'lanes': [40, 9, 33]}[where]
    A = torch.zeros(1024, 4)
    A[:, 0], A[:, 2] = 500.0, 510.0                                                   # everything else is far away
    A[:, 1] = torch.arange(1024) * 10.0
    A[:, 3] = A[:, 1] + 10
    A[cols] = torch.tensor([0.0, 0, 10, 10])
    gb, gc = torch.tensor([[[0.0, 0, 10, 20]]]), torch.tensor([[2]])
    out = _label(A, gb, gc, thr=0.6)
    assert (out[1][0] >= 0).nonzero().flatten().tolist() == [min(cols)]
    _check_against_oracle(A, gb, gc, out, thr=0.6)
    out = _label(A, gb, gc, thr=0.5)
    assert (out[1][0] >= 0).nonzero().flatten().tolist() == sorted(cols)
    _check_against_oracle(A, gb, gc, out, thr=0.5)


def test_many_rows_on_one_column():
    """300 identical rows (different labels) and a few others: every identical row claims the same column, only row 0 owns
    it, and no anchor anywhere is matched to rows 1..299; two different rows share their best anchor too (lowest row wins)"""
    A = _std_anchors(128)
    M = 306
    gb = torch.zeros(2, M, 4)
    gc = torch.zeros(2, M, dtype=torch.int64)
    gb[:, :300] = torch.tensor([30.0, 30, 70, 80])
    gc[:, :300] = (torch.arange(300) % 6 + 1)
    gb[0, 300:] = torch.tensor([[20.0, 20, 52, 52], [21, 21, 51, 51], [90, 10, 120, 50], [2000, 2000, 2040, 2040], [40, 40, 40, 40],
                                [5, 90, 25, 120]])
    gc[0, 300:] = torch.tensor([1, 2, 3, 4, 5, 6])
    gb[1, 300:] = gb[0, 300:].flip(0)
    gc[1, 300:] = gc[0, 300:].flip(0)
    out = _label(A, gb, gc)
    match = _check_against_oracle(A, gb, gc, out)
    for b in range(2):
        seen = set(match[b].unique().tolist())
        assert 0 in seen and not seen & set(range(1, 300))
        assert int(out[2][b][match[b] == 0][0]) == 0                                  # label of row 0, minus one
    # rows 303 / 304 of image 0 (no overlap, zero area) and rows 0..299 do not compete for anchor 0; row 303 < 304 gets it
    assert int(match[0][0]) == 303 and int(match[1][0]) == 301


def test_degenerate_boxes():
    """valid input the kernel must take without surprises: y2 < y0 (intersection clamps to 0: IoU 0, forced onto anchor 0, the
    encode takes the log of a negative quotient: NaN, on both sides), coordinates of 1e6, a box that covers everything"""
    A = _std_anchors(128)
    gb = torch.tensor([[[30.0, 30, 70, 80], [50, 50, 20, 80], [1e6, 1e6, 1e6 + 50, 1e6 + 50], [-1e6, -1e6, 1e6, 1e6], [60, 60, 100, 20]],
                       [[50, 50, 20, 80], [30.0, 30, 70, 80], [-1e6, -1e6, 1e6, 1e6], [0, 0, 0, 0], [1e6, 0, 1e6 + 1, 128]]])
    gc = torch.tensor([[1, 2, 3, 4, 5], [6, 5, 4, 3, 2]])
    out = _label(A, gb, gc)
    _check_against_oracle(A, gb, gc, out)
    assert int(out[1][0][0]) == 1 and bool(torch.isnan(out[3][0][0][2]))               # the y2 < y0 row owns anchor 0
    assert int(out[1][1][0]) == 0


# ------------------------------------------------------------------------------------------------ workspace
def test_workspace_one_byte_short_is_rejected():
    A = _std_anchors(128)
    gb, gc = torch.tensor([[[30.0, 30, 70, 80]]]), torch.tensor([[1]])
    bufs = Buffers(1, 1, A.shape[0])
    assert bufs.nbytes == A.shape[0] * 8 + 1 * ((A.shape[0] + 255) // 256) * 8
    for rows in (False, True):
        assert _label(A, gb, gc, rows=rows, bufs=bufs, nbytes=bufs.nbytes - 1)[0] == -22
    assert int(bufs.cls_t[0, 0]) == 77                                                 # nothing was written
    assert _label(A, gb, gc, bufs=bufs)[0] == 0


def test_second_call_on_the_same_buffers_carries_nothing_over():
    """num_positives and the force table are cleared by the entry point itself"""
    from _seeded import label_case
    A = _std_anchors(640)
    B, Mmax = 4, 64
    bufs = Buffers(B, Mmax, A.shape[0])
    gb1, gc1 = label_case(5, B, Mmax, 640)
    _check_against_oracle(A, gb1, gc1, _label(A, gb1, gc1, bufs=bufs))
    gb2, gc2 = label_case(6, B, Mmax, 640)
    gb2, gc2 = gb2[::-1].copy(), gc2[::-1].copy()                                      # the full image where the empty one was
    _check_against_oracle(A, gb2, gc2, _label(A, gb2, gc2, bufs=bufs))
    gb3, gc3 = np.zeros_like(gb1), np.full_like(gc1, -1)                               # nothing at all
    rc, match, cls_t, box_t, npos = _label(A, gb3, gc3, bufs=bufs)
    assert rc == 0 and bool((match == -1).all()) and bool((cls_t == -1).all()) and not bool(box_t.any()) and not bool(npos.any())


# ------------------------------------------------------------------------------------------------ relabelling
def _threshold_neighbours():
    """against [0, 0, 100, 100]: the integer box [0, 0, 100, 90] has IoU 9000 / 10000 = float32(0.9) exactly; 0.9 has no
    float32 neighbour that integer boxes reach, so the nearest IoU value on each side is taken from the oracle's own IoU over
    the shifted boxes [0, d, 100, 100 + d], d among the float32 neighbours of 100 / 19 (IoU = (100 - d) / (100 + d)).  They
    turn out to be exactly one float32 step above and one below 0.9."""
    t = torch.tensor([[0.0, 0, 100, 100]])
    at = torch.tensor([0.0, 0, 100, 90])
    thr = torch.tensor(0.9, dtype=torch.float32)
    assert float(ot.iou_yxyx(t, at[None])[0, 0]) == float(thr)
    d = np.float32(100.0 / 19.0)
    ds = [d]
    lo = hi = d
    for _ in range(60):
        lo, hi = np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(100))
        ds += [lo, hi]
    cand = torch.tensor([[0.0, float(v), 100.0, float(np.float32(100) + v)] for v in ds])
    iou = ot.iou_yxyx(t, cand)[0]
    above = cand[iou > thr][iou[iou > thr].argmin()]
    below = cand[iou < thr][iou[iou < thr].argmax()]
    one_up, one_down = np.nextafter(np.float32(0.9), np.float32(1)), np.nextafter(np.float32(0.9), np.float32(0))
    assert float(ot.iou_yxyx(t, above[None])[0, 0]) == float(one_up) and float(ot.iou_yxyx(t, below[None])[0, 0]) == float(one_down)
    return at, above, below


def _relabel(gb, gc, task):
    import _hip
    from ood_object_detection_amd import _lib
    lib = _lib.load()
    gbd = torch.as_tensor(gb, dtype=torch.float32).to(DEV).contiguous()
    gcd = torch.as_tensor(gc, dtype=torch.int64).to(DEV).contiguous()
    B, Mmax = gcd.shape
    rc = lib.effdet_relabel_task_cls(_hip.stream(DEV), gbd.data_ptr(), gcd.data_ptr(), B, Mmax, task, 0.9)
    torch.cuda.synchronize()
    return rc, gcd.cpu()


@pytest.mark.parametrize('Mmax', [1, 37, 512])
def test_relabel_task_cls_vs_oracle(Mmax):
    """seeded images: task boxes with near copies on either side of IoU 0.9 (shrunk by 0 to 20 % in one direction), the
    constructed boxes at IoU exactly 0.9 and one float32 step above / below it, images without the task class, images of the
    task class only, rows of class -1; the device rewrites gt_cls in place exactly as the oracle says"""
    task = 3
    at, above, below = _threshold_neighbours()
    rs = np.random.RandomState(40 + Mmax)
    B = 8
    gb = np.zeros((B, Mmax, 4), np.float32)
    gc = np.full((B, Mmax), -1, np.int64)
    others = [1, 2, -1, 5]
    for b in range(B):
        mode = {1: 'task only', 2: 'no task'}.get(b, 'mixed')
        n = Mmax if b < 3 else rs.randint(0, Mmax + 1)
        tasks = []                                                   # boxes that near copies are made of
        for p in np.sort(rs.permutation(Mmax)[:n]):
            r = rs.uniform()
            if mode == 'task only' or not tasks or r < 0.3:
                h, w = rs.uniform(20, 200, 2)
                y0, x0 = rs.uniform(300, 700, 2)                     # clear of the constructed boxes at the origin
                gb[b, p] = (y0, x0, y0 + h, x0 + w)
                is_task = mode == 'task only' or (mode == 'mixed' and (not tasks or r < 0.15))
                gc[b, p] = task if is_task else others[rs.randint(0, 4)]
                if is_task or mode == 'no task':
                    tasks.append(gb[b, p].copy())
            else:
                t = tasks[rs.randint(0, len(tasks))]
                gb[b, p] = t
                gb[b, p, 3] = t[1] + (t[3] - t[1]) * rs.uniform(0.8, 1.0)      # IoU with t = the factor, 0.8 .. 1.0
                gc[b, p] = others[rs.randint(0, 4)]
    if Mmax >= 37:                                                   # image 0: the constructed threshold cases
        for k, (box, c) in enumerate([(np.array([0, 0, 100, 100], np.float32), task), (at.numpy(), 5), (above.numpy(), 6),
                                      (below.numpy(), 7)]):
            gb[0, 4 * k + 1], gc[0, 4 * k + 1] = box, c
    rc, new = _relabel(gb, gc, task)
    assert rc == 0
    changed = 0
    for b in range(B):
        ref = ot.relabel_task_cls(torch.from_numpy(gb[b]), torch.from_numpy(gc[b]), task)
        assert torch.equal(new[b], ref), b
        changed += int((ref != torch.from_numpy(gc[b])).sum())
    assert torch.equal(new[2], torch.from_numpy(gc[2])) and torch.equal(new[1], torch.from_numpy(gc[1]))
    if Mmax >= 37:
        assert changed > 0
        # exactly 0.9 and the step below stay, the step above is relabelled
        t = torch.from_numpy(gb[0, 1:2])
        iou = [float(ot.iou_yxyx(t, torch.from_numpy(gb[0, 4 * k + 1:4 * k + 2]))[0, 0]) for k in (1, 2, 3)]
        f9 = float(np.float32(0.9))
        assert iou[0] == f9 and iou[1] > f9 > iou[2]
        assert [int(new[0, 4 * k + 1]) for k in (1, 2, 3)] == [5, task, 7]


def test_relabel_rejects_bad_sizes():
    gb, gc = np.zeros((1, 513, 4), np.float32), np.ones((1, 513), np.int64)
    assert _relabel(gb, gc, 3)[0] == -22
    assert _relabel(gb[:, :4], gc[:, :4], -1)[0] == -22


def test_log_deviation_report():
    """Runs last in this file: the largest th / tw deviation the tests above saw, in float32 ulps at max(|ref|, 1), against
    the 2-ulp bound each of them asserted.  Measured on an MI355X: 1.8035 ulps (also in DESIGN.md, labeler paragraph)."""
    print('largest th / tw deviation: %.4f float32 ulps (bound 2)' % _worst_log_ulps[0])
    assert _worst_log_ulps[0] <= 2.0
