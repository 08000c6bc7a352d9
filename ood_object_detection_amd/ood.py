"""OOD evaluation helpers on the device.

The class head emits per-anchor `energy = -logsumexp_c z` and `max_logit = max_c z`.  For the
in-distribution-vs-OOD experiment an image is scored by `max_a(-energy_a)` and the separation is reported as
AUROC; both run as HIP kernels so that nothing but two integers leaves the GPU.

Detection-level evaluation (`detection_metrics`, `OODEvaluator`): AUROC, AUPR with either class as the positive one and FPR at a
TPR level over per-detection or per-anchor scores, 10^5 ... 10^7 a side.  The scores are compacted into device buffers, sorted
by a radix sort and evaluated by binary searches (csrc/ood_eval.hip); one block of 96 bytes leaves the GPU."""
import struct

import torch

from . import _lib


def image_scores(anchor_energy: torch.Tensor) -> torch.Tensor:
    """[B, N] float32 per-anchor energies (model.ood_energy) -> [B] image-level scores max_a(-energy)."""
    if anchor_energy.device.type != 'cuda' or anchor_energy.dtype != torch.float32 or anchor_energy.dim() != 2:
        raise RuntimeError('expected a float32 [B, N] GPU tensor (no CPU fallback)')
    lib = _lib.load()
    e = anchor_energy.contiguous()
    out = torch.empty(e.shape[0], dtype=torch.float32, device=e.device)
    st = torch.cuda.current_stream(e.device).cuda_stream
    _lib.check(lib.effdet_ood_image_score(st, e.data_ptr(), e.shape[0], e.shape[1], out.data_ptr()), 'effdet_ood_image_score')
    return out


def auroc(in_dist_scores: torch.Tensor, ood_scores: torch.Tensor) -> float:
    """AUROC with the in-distribution images as the positive class (exact pair counting, ties count 1/2)."""
    for t in (in_dist_scores, ood_scores):
        if t.device.type != 'cuda' or t.dtype != torch.float32 or t.dim() != 1 or t.numel() == 0:
            raise RuntimeError('expected non-empty float32 1-d GPU tensors (no CPU fallback)')
    lib = _lib.load()
    pos, neg = in_dist_scores.contiguous(), ood_scores.contiguous()
    counts = torch.empty(2, dtype=torch.int64, device=pos.device)
    st = torch.cuda.current_stream(pos.device).cuda_stream
    _lib.check(lib.effdet_auroc_counts(st, pos.data_ptr(), neg.data_ptr(), pos.numel(), neg.numel(), counts.data_ptr()),
               'effdet_auroc_counts')
    gt, eq = counts.tolist()
    return (gt + 0.5 * eq) / (pos.numel() * neg.numel())


def novelty_score(proj_embds: torch.Tensor, confs: torch.Tensor, proto_idx: torch.Tensor, dot_mult: float, dot_add: float,
                  sim_target: str = 'avg'):
    """The fork's own novelty score (infer.py:425-427, 465-471, 607-616), one HIP launch: for every anchor
    `sigmoid(dot_mult * (conf + dot_add)) * sim`, sim = mean ('avg') or max ('max') cosine similarity of its ProjectionNet
    embedding to the cluster prototypes `proto_idx` (the episode code's `max_idxs`).
    proj_embds [n, d] float32 (un-normalised ProjectionNet outputs), confs [n] anchor confidence logits.
    Returns dict(score, soft_thresh, sim), each [n] float32."""
    if proj_embds.device.type != 'cuda' or proj_embds.dtype != torch.float32 or proj_embds.dim() != 2:
        raise RuntimeError('expected float32 [n, d] GPU embeddings (no CPU fallback)')
    if sim_target not in ('avg', 'max'):
        raise ValueError("sim_target must be 'avg' or 'max' (infer.py FLAGS.sim_target)")
    lib = _lib.load()
    e = proj_embds.detach().contiguous()
    n, d = e.shape
    c = confs.detach().to(device=e.device, dtype=torch.float32).reshape(n).contiguous()
    pi = proto_idx.to(device=e.device, dtype=torch.int64).reshape(-1).contiguous()
    m = pi.numel()
    if m == 0 or m * d > 16384:
        raise ValueError('between 1 and 16384 / d prototypes')
    out = torch.empty(3, n, dtype=torch.float32, device=e.device)
    st = torch.cuda.current_stream(e.device).cuda_stream
    _lib.check(lib.effdet_novelty_score(st, e.data_ptr(), c.data_ptr(), pi.data_ptr(), n, d, m, float(dot_mult), float(dot_add),
                                        1 if sim_target == 'max' else 0, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr()),
               'effdet_novelty_score')
    return {'score': out[0], 'soft_thresh': out[1], 'sim': out[2]}


_FLAG_TEXT = ((1, 'a NaN among the in-distribution scores'), (2, 'the in-distribution capacity overflowed'),
              (4, 'a NaN among the OOD scores'), (8, 'the OOD capacity overflowed'),
              (16, 'the in-distribution side is empty'), (32, 'the OOD side is empty'))


def _check_level(recall_level):
    if not (0.0 < float(recall_level) <= 1.0):
        raise ValueError('recall_level must lie in (0, 1], got %r' % (recall_level,))
    return float(recall_level)


def _check_scores(t, what):
    if not torch.is_tensor(t) or t.device.type != 'cuda' or t.dtype != torch.float32:
        raise RuntimeError('%s: expected a float32 GPU tensor (no CPU fallback)' % what)


class OODEvaluator:
    """Accumulates in-distribution and OOD scores on the device (a higher score = more in-distribution, e.g. `-energy`) and
    evaluates AUROC, AUPR in / out and FPR at a TPR level.  Nothing synchronises with the host before `evaluate`, and `add`,
    `add_detections` and the device part of `evaluate` (`enqueue`) can be captured in a `torch.cuda.graph`.
    capacity_in / capacity_ood: the most scores a side can hold (<= 2^27); appending more is reported by `evaluate`.
    storage: optional pair of caller-owned 1-d float32 GPU tensors (at least the capacities long) to accumulate in."""

    MAX_SCORES = 1 << 27

    def __init__(self, capacity_in, capacity_ood, device='cuda', storage=None):
        self.capacity = (int(capacity_in), int(capacity_ood))
        if min(self.capacity) < 1 or max(self.capacity) > self.MAX_SCORES:
            raise ValueError('capacities must lie in [1, 2^27], got %r' % (self.capacity,))
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('OODEvaluator runs on the GPU (no CPU fallback)')
        self._storage = storage
        self._bufs = None

    def _setup(self):
        if self._bufs is not None:
            return
        lib = _lib.load()
        dev = self.device
        if self._storage is not None:
            bufs = list(self._storage)
            for b, c in zip(bufs, self.capacity):
                _check_scores(b, 'storage')
                if b.dim() != 1 or not b.is_contiguous() or b.numel() < c:
                    raise ValueError('storage: contiguous 1-d tensors of at least the capacity')
        else:
            bufs = [torch.empty(c, dtype=torch.float32, device=dev) for c in self.capacity]
        self._ws_bytes = lib.effdet_ood_eval_workspace_bytes(*self.capacity)
        if self._ws_bytes <= 0:
            raise RuntimeError('effdet_ood_eval_workspace_bytes failed with code %d' % self._ws_bytes)
        self._ws = torch.empty(self._ws_bytes, dtype=torch.uint8, device=dev)
        self._sorted_off = [lib.effdet_ood_eval_sorted_offset(*self.capacity, s) for s in (0, 1)]
        self._state = torch.zeros(4, dtype=torch.int32, device=dev)        # {cursor, flags} of each side
        self._result = torch.zeros(12, dtype=torch.int64, device=dev)
        self._counts = None
        self._bufs = bufs

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def clear(self):
        """Forget every score (a device-side reset, no synchronisation)."""
        self._setup()
        self._state.zero_()
        self._counts = None

    def _append(self, scores, ood, count, det_scores, min_score, negate):
        _check_scores(scores, 'scores')
        if scores.dim() not in (1, 2):
            raise ValueError('scores must be 1-d or [B, K]')
        self._setup()
        lib = _lib.load()
        s2 = scores.detach()
        s2 = s2.reshape(1, -1) if s2.dim() == 1 else s2
        B, K = s2.shape
        if B == 0 or K == 0:
            return
        if B * K > self.MAX_SCORES:
            raise ValueError('at most 2^27 entries per call')
        cnt_ptr, cnt64 = None, 0
        if count is not None:
            if count.device != s2.device or count.dtype not in (torch.int32, torch.int64) or count.numel() != B:
                raise ValueError('count: an int32 or int64 tensor of B entries on the device of the scores')
            count = count.detach().reshape(B).contiguous()
            cnt_ptr, cnt64 = count.data_ptr(), int(count.dtype == torch.int64)
        det_ptr, det_pitch, det_stride = None, 0, 0
        if det_scores is not None:
            _check_scores(det_scores, 'det_scores')
            if tuple(det_scores.shape) != (B, K) or det_scores.device != s2.device or min_score is None:
                raise ValueError('det_scores must be [B, K] like the scores and come with a min_score')
            det_scores = det_scores.detach()
            if min(det_scores.stride()) < 0:
                det_scores = det_scores.contiguous()
            det_ptr, (det_pitch, det_stride) = det_scores.data_ptr(), det_scores.stride()
        if min(s2.stride()) < 0:
            s2 = s2.contiguous()
        side = 1 if ood else 0
        _lib.check(lib.effdet_ood_eval_append(self._stream(), s2.data_ptr(), s2.stride(0), s2.stride(1), B, K, cnt_ptr, cnt64,
                                              det_ptr, det_pitch, det_stride, float(min_score) if min_score is not None else 0.0,
                                              1 if negate else 0, self._bufs[side].data_ptr(), self.capacity[side],
                                              self._state[2 * side:].data_ptr(), self._ws.data_ptr(), self._ws_bytes),
                   'effdet_ood_eval_append')
        self._counts = None

    def add(self, scores, ood):
        """Append every entry of a 1-d or 2-d float32 GPU tensor to the OOD (`ood=True`) or the in-distribution side."""
        self._append(scores, ood, None, None, None, False)

    def add_detections(self, scores, count, ood, det_scores=None, min_score=None, negate=False):
        """Append the valid entries of a [B, K] tensor of `DetBenchPredict.last_ood` (`energy`, `max_logit`; strided views
        are fine): entry (b, j) counts when j < count[b] (`DetBenchPredict.last_count`; None: all K) and, if `det_scores`
        [B, K] (e.g. `det[..., 4]`) is given, when its detection score is >= min_score.  negate: append `-scores` (an energy
        becomes a score)."""
        if scores.dim() != 2:
            raise ValueError('scores must be [B, K]')
        self._append(scores, ood, count, det_scores, min_score, negate)

    def enqueue(self, recall_level=0.95):
        """The device part of `evaluate`: sort + metrics on the current stream, no synchronisation (14 launches)."""
        level = _check_level(recall_level)
        self._setup()
        lib = _lib.load()
        st = self._stream()
        _lib.check(lib.effdet_ood_eval_sort(st, self._bufs[0].data_ptr(), self.capacity[0], self._bufs[1].data_ptr(), self.capacity[1],
                                            self._state.data_ptr(), self._ws.data_ptr(), self._ws_bytes), 'effdet_ood_eval_sort')
        _lib.check(lib.effdet_ood_eval_metrics(st, self.capacity[0], self.capacity[1], self._state.data_ptr(), self._ws.data_ptr(),
                                               self._ws_bytes, level, self._result.data_ptr()), 'effdet_ood_eval_metrics')

    def result(self):
        """Read the result block of the last `enqueue` (synchronises) -> dict; ValueError names an empty side, a NaN or an
        overflown capacity."""
        self._setup()
        raw = self._result.cpu().numpy().tobytes()
        P, N, gt, eq, tp, fp, flags, _k = struct.unpack_from('<8Q', raw, 0)
        aupr_in, aupr_out = struct.unpack_from('<2d', raw, 64)
        threshold, = struct.unpack_from('<f', raw, 80)
        if flags:
            raise ValueError('OOD evaluation: ' + '; '.join(text for bit, text in _FLAG_TEXT if flags & bit))
        self._counts = (P, N)
        return {'auroc': (gt + 0.5 * eq) / (P * N), 'aupr_in': aupr_in, 'aupr_out': aupr_out, 'fpr_at_tpr': fp / N, 'tpr': tp / P,
                'threshold': threshold, 'tp': tp, 'fp': fp, 'pairs_gt': gt, 'pairs_eq': eq, 'n_in': P, 'n_ood': N}

    def threshold_tensor(self):
        """The `threshold` of the last `enqueue` where it lies on the device: a 0-d float32 view of the result block (word 10, low
        half), so `enqueue`, `relabel_unknown` and an evaluator's `add_batch` chain without a host read and capture together."""
        self._setup()
        return self._result.view(torch.float32)[20]

    def evaluate(self, recall_level=0.95):
        """Sort both sides and evaluate; the only call that synchronises.  Returns dict(auroc, aupr_in, aupr_out, fpr_at_tpr,
        tpr, threshold, tp, fp, pairs_gt, pairs_eq, n_in, n_ood): in-distribution is the positive class of auroc / aupr_in,
        OOD of aupr_out; fpr_at_tpr is the share of OOD scores at or above the largest threshold that keeps
        tpr >= recall_level."""
        self.enqueue(recall_level)
        return self.result()

    def sorted_scores(self):
        """(in-distribution, OOD) scores in ascending order: device views into the workspace, valid after `evaluate` until the
        next `add` / `evaluate`."""
        if self._bufs is None or self._counts is None:
            raise RuntimeError('sorted_scores() follows evaluate()')
        return tuple(self._ws[off:off + 4 * n].view(torch.float32) for off, n in zip(self._sorted_off, self._counts))


def relabel_unknown(det, count, scores, threshold, num_classes, out=None):
    """Detections whose in-distribution score misses the threshold become the unknown class `num_classes + 1` (one launch):
    det [B, max_det, 6] float32 rows x1,y1,x2,y2,score,class (1-based); row (b, j) gets class num_classes + 1 where j < count[b],
    its class is in 1..num_classes and not scores[b, j] >= threshold (a NaN score becomes unknown); every other row is copied.
    scores: [B, max_det] float32, any non-negative strides (a view of `DetBenchPredict.last_ood`, `-energy`, ...).  threshold: a
    float, or a 0-d float32 GPU tensor read on the device (`OODEvaluator.threshold_tensor()`).  out: the tensor to write, `det`
    itself for in-place use; None allocates one."""
    for t, what in ((det, 'det'), (scores, 'scores')):
        _check_scores(t, what)
    if det.dim() != 3 or det.shape[2] != 6 or not det.is_contiguous():
        raise ValueError('det must be a contiguous [B, max_det, 6] tensor')
    B, max_det, _ = det.shape
    if tuple(scores.shape) != (B, max_det) or scores.device != det.device:
        raise ValueError('scores must be [B, max_det] on the device of det')
    if not 1 <= int(num_classes) <= 65534:
        raise ValueError('num_classes must lie in [1, 65534]')
    if not torch.is_tensor(count) or count.device != det.device or count.numel() != B:
        raise ValueError('count: a tensor of B entries on the device of det')
    count = count.detach().reshape(B).to(torch.int32).contiguous()
    scores = scores.detach()
    if min(scores.stride()) < 0:
        scores = scores.contiguous()
    tau, tau_ptr = 0.0, None
    if torch.is_tensor(threshold):
        if threshold.device != det.device or threshold.dtype != torch.float32 or threshold.numel() != 1:
            raise ValueError('threshold: a float or a 0-d float32 tensor on the device of det')
        tau_ptr = threshold.data_ptr()
    else:
        tau = float(threshold)
    if out is None:
        out = torch.empty_like(det)
    elif out.device != det.device or out.dtype != torch.float32 or out.shape != det.shape or not out.is_contiguous():
        raise ValueError('out must be a contiguous float32 tensor like det')
    if B * max_det:
        st = torch.cuda.current_stream(det.device).cuda_stream
        _lib.check(_lib.load().effdet_relabel_unknown(st, det.data_ptr(), count.data_ptr(), scores.data_ptr(), scores.stride(0),
                                                      scores.stride(1), B, max_det, int(num_classes), tau, tau_ptr, out.data_ptr()),
                   'effdet_relabel_unknown')
    return out


def detection_metrics(in_dist_scores: torch.Tensor, ood_scores: torch.Tensor, recall_level: float = 0.95):
    """AUROC, AUPR in / out and FPR at `recall_level` TPR of two 1-d float32 GPU tensors of scores (higher = more
    in-distribution; see `OODEvaluator.evaluate` for the dict)."""
    _check_level(recall_level)
    for t in (in_dist_scores, ood_scores):
        _check_scores(t, 'scores')
        if t.dim() != 1:
            raise RuntimeError('expected 1-d tensors')
    empty = (16 if in_dist_scores.numel() == 0 else 0) | (32 if ood_scores.numel() == 0 else 0)
    if empty:
        raise ValueError('OOD evaluation: ' + '; '.join(text for bit, text in _FLAG_TEXT if empty & bit))
    ev = OODEvaluator(in_dist_scores.numel(), ood_scores.numel(), in_dist_scores.device)
    ev.add(in_dist_scores, False)
    ev.add(ood_scores, True)
    return ev.evaluate(recall_level)
