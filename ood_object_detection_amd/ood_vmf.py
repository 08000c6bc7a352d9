"""The von Mises-Fisher hyperspherical OOD head on the device (csrc/vmf.hip): SIREN (Du, Gozum, Ming, Li, NeurIPS
2022) shapes the REPRESENTATION of the class head, where `ood_train.EnergyRegularizer` shapes its logits.  A bias-free MLP projects
the class tower of every pyramid cell to d dimensions; on the unit sphere every class is a von Mises-Fisher density with a
prototype mu_c (an exponential moving average of the class's unit embeddings, not differentiated) and a learnable concentration
kappa_c = exp(log_kappa_c), and the head trains with the vMF log-likelihood:

    head = VMFHead(config.fpn_channels, config.num_classes, num_anchors, dim=64)
    tower = engine.class_penultimate(tower=True)                  # per-level [B, F, h, w]
    loss, stats = head(tower, cls_targets)                        # EMA update of the prototypes, then the loss; one autograd node

    scorer = VMFFeatureOOD(head)
    bench = DetBenchPredict(model, feature_ood=[scorer])          # last_ood gains vmf, vmf_class, vmf_cosine
    knn.add(scorer.embeddings(tower)); knn.score(scorer.embeddings(tower, anchor_index, count), ...)     # SIREN's k-NN variant

With u the embedding of an anchor's cell, r = u / max(|u|, 1e-12), nu = d / 2 - 1 and Z_d(kappa) = kappa^nu / ((2 pi)^(d/2) I_nu(kappa)):

    l_c = log Z_d(kappa_c) + kappa_c mu_c . r  over the classes that have a prototype;  loss = mean_i (logsumexp_c l_ic - l_iy)
    vmf = max_c l_c,  vmf_class = the lowest class that attains it,  vmf_cosine = max_c mu_c . r

log I_nu(kappa) and the Bessel ratio of the gradient are evaluated on the device in float64 (a series of positive terms, a thread per
class): nothing synchronises with the host, everything can be captured in a graph and gives the same bits every run.  An anchor
counts when its label lies in [0, C); one whose embedding holds a non-finite value is skipped and counted in `stats['skipped']`.
The paper's projection head has biases; this one has none, because it runs on `meta_ops.ProjLinear`.  There is no CPU fallback.

The prototype update is sequential per class by definition (every row moves the mean the next row sees).  A wave per class walks
its rows in (b, j) order; `ema_rows_per_class` bounds the chain (DESIGN.md §8 has the measurement)."""
import math

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib
from .ood_features import _PyramidRows, WIDTHS

MAX_CLASSES = 1024
MAX_DIM = 256
MAX_ROWS = 1 << 27
KAPPA_MIN, KAPPA_MAX = 2.0 ** -7, 2.0 ** 13
STAT_KEYS = ('m', 'skipped', 'valid_classes', 'mean_cosine', 'mean_kappa', 'max_kappa', 'loss64')


def _ws(lib, rows, C, d, dev):
    n = lib.effdet_vmf_workspace_bytes(rows, C, d)
    if n <= 0:
        raise ValueError('between 1 and 2^27 rows per call, got %d' % rows)
    return torch.empty(n, dtype=torch.uint8, device=dev), n


def partition(log_kappa, dim):
    """log_kappa [C] float32 (GPU) -> dict of device tensors: kappa, logz (float32), logz64, ratio (float64), clamped (int32)"""
    if log_kappa.device.type != 'cuda':
        raise RuntimeError('vmf partition: log_kappa must be a GPU tensor (no CPU fallback)')
    if log_kappa.dim() != 1 or log_kappa.dtype != torch.float32 or not 1 <= log_kappa.numel() <= MAX_CLASSES or not 2 <= int(dim) <= MAX_DIM:
        raise ValueError('log_kappa: float32 [C] with 1 <= C <= %d; 2 <= dim <= %d' % (MAX_CLASSES, MAX_DIM))
    th = log_kappa.detach().contiguous()
    C, dev = th.numel(), th.device
    out = {'kappa': torch.empty(C, dtype=torch.float32, device=dev), 'logz': torch.empty(C, dtype=torch.float32, device=dev),
           'logz64': torch.empty(C, dtype=torch.float64, device=dev), 'ratio': torch.empty(C, dtype=torch.float64, device=dev),
           'clamped': torch.empty(C, dtype=torch.int32, device=dev)}
    _lib.check(_lib.load().effdet_vmf_partition(torch.cuda.current_stream(dev).cuda_stream, th.data_ptr(), C, int(dim), out['kappa'].data_ptr(),
                                                out['logz'].data_ptr(), out['logz64'].data_ptr(), out['ratio'].data_ptr(),
                                                out['clamped'].data_ptr()), 'effdet_vmf_partition')
    return out


def _labels(cls_targets, B, K, dev):
    if not torch.is_tensor(cls_targets):
        from .effdet.loss import _pack_targets
        cls_targets = _pack_targets(list(cls_targets), 0)
    t = cls_targets.detach()
    if t.dim() != 2 or tuple(t.shape) != (B, K):
        raise ValueError('cls_targets: the per-level [B, H, W, A] list or a [%d, %d] tensor, got %s' % (B, K, tuple(t.shape)))
    if t.dtype not in (torch.int32, torch.int64, torch.float32):
        raise ValueError('cls_targets must be int32, int64 or float32')
    if t.device != dev:
        raise RuntimeError('cls_targets must live on the device of the embeddings')
    if min(t.stride()) < 0:
        t = t.contiguous()
    return t, ({torch.int32: 0, torch.int64: 1, torch.float32: 2}[t.dtype], t.stride(0), t.stride(1), 0)


def update_prototypes(U, labels, num_anchors, prototypes, valid, ema=0.95, rows_per_class=None):
    """The ordered EMA update in place: U [B, P, d] float32, labels [B, A * P], prototypes [C, d] float32, valid [C] int32."""
    lib = _lib.load()
    B, P, d = U.shape
    C, A = prototypes.shape[0], int(num_anchors)
    lab, largs = _labels(labels, B, A * P, U.device)
    ws, n = _ws(lib, B * A * P, C, d, U.device)
    _lib.check(lib.effdet_vmf_update(torch.cuda.current_stream(U.device).cuda_stream, U.data_ptr(), B, P, A, d, lab.data_ptr(), *largs, C,
                                     float(ema), int(rows_per_class or 0), prototypes.data_ptr(), valid.data_ptr(), ws.data_ptr(), n),
               'effdet_vmf_update')


class _VMFLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, U, log_kappa, labels, head, update):
        lib = _lib.load()
        U = U.contiguous()
        B, P, d = U.shape
        C, A, dev = head.C, head.A, U.device
        part = partition(log_kappa, d)
        lab, largs = _labels(labels, B, A * P, dev)
        if update:
            update_prototypes(U.detach(), lab, A, head.prototypes, head.valid, head.ema, head.ema_rows_per_class)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        stats = torch.empty(8, dtype=torch.float64, device=dev)
        dU = torch.empty_like(U)
        dth = torch.empty(C, dtype=torch.float32, device=dev)
        ws, n = _ws(lib, B * A * P, C, d, dev)
        _lib.check(lib.effdet_vmf_loss(torch.cuda.current_stream(dev).cuda_stream, U.data_ptr(), B, P, A, d, lab.data_ptr(), *largs, C,
                                       head.prototypes.data_ptr(), head.valid.data_ptr(), part['kappa'].data_ptr(), part['logz'].data_ptr(),
                                       part['ratio'].data_ptr(), part['clamped'].data_ptr(), loss.data_ptr(), stats.data_ptr(),
                                       dU.data_ptr(), dth.data_ptr(), ws.data_ptr(), n), 'effdet_vmf_loss')
        ctx.save_for_backward(dU, dth)
        ctx.mark_non_differentiable(stats)
        return loss[0].clone(), stats

    @staticmethod
    @once_differentiable                                        # a second-order backward is not built: differentiating twice raises
    def backward(ctx, g_loss, _g_stats):
        dU, dth = ctx.saved_tensors
        gU = dU * g_loss.to(dU.dtype) if ctx.needs_input_grad[0] else None
        gt = dth * g_loss.to(dth.dtype) if ctx.needs_input_grad[1] else None
        return gU, gt, None, None, None


class VMFHead(nn.Module):
    """The projection MLP (two bias-free Linear weights, F -> hidden -> dim), log_kappa [C] and the buffers prototypes [C, dim] and
    valid [C] (module docstring).  num_features: the width of the class tower (64, 88, 112, 160, 224 or 288); 1 <= num_classes <= 1024;
    num_anchors: anchors per cell (A), anchor n sits on cell n // A; 2 <= dim <= 256; hidden: None = num_features; kappa_init in
    [2^-7, 2^13]; ema: the weight alpha of the old prototype; ema_rows_per_class: at most that many rows of a class move its
    prototype in one call (None: all).  The chain of a class is sequential, about 0.85 us a row on an MI355X: a class that holds
    several thousand rows of a step costs more than the loss kernels do, so 64 is the recommended value where a class dominates
    (DESIGN.md §8 has the measurement).
    forward(levels, cls_targets, update=True) -> (loss, stats): levels the per-level [B, F, h, w] list (or a [B, P, F] tensor),
    cls_targets the labeler's per-level [B, H, W, A] list or a packed [B, A * P] tensor; stats: a dict of device tensors."""

    def __init__(self, num_features, num_classes, num_anchors, dim=64, hidden=None, kappa_init=10.0, ema=0.95, ema_rows_per_class=None):
        super().__init__()
        self.F, self.C, self.A, self.dim = int(num_features), int(num_classes), int(num_anchors), int(dim)
        self.hidden = self.F if hidden is None else int(hidden)
        if self.F not in WIDTHS:
            raise ValueError('num_features must be one of %r, got %d' % (WIDTHS, self.F))
        if not 1 <= self.C <= MAX_CLASSES:
            raise ValueError('num_classes must lie in [1, %d], got %d' % (MAX_CLASSES, self.C))
        if self.A < 1:
            raise ValueError('num_anchors must be >= 1')
        if not 2 <= self.dim <= MAX_DIM:
            raise ValueError('dim must lie in [2, %d], got %d' % (MAX_DIM, self.dim))
        if self.hidden < 1:
            raise ValueError('hidden must be >= 1')
        if not KAPPA_MIN <= float(kappa_init) <= KAPPA_MAX:
            raise ValueError('kappa_init must lie in [2^-7, 2^13], got %r' % (kappa_init,))
        self.ema = float(ema)
        if not 0.0 <= self.ema <= 1.0:
            raise ValueError('ema must lie in [0, 1], got %r' % (ema,))
        if ema_rows_per_class is not None and int(ema_rows_per_class) < 1:
            raise ValueError('ema_rows_per_class must be None or >= 1')
        self.ema_rows_per_class = None if ema_rows_per_class is None else int(ema_rows_per_class)
        g = torch.Generator().manual_seed(0)
        init = lambda n, k: nn.Parameter((torch.rand(n, k, generator=g) * 2 - 1) / math.sqrt(k))      # nn.Linear's range
        self.weight1, self.weight2 = init(self.hidden, self.F), init(self.dim, self.hidden)
        self.log_kappa = nn.Parameter(torch.full((self.C,), math.log(float(kappa_init))))
        self.register_buffer('prototypes', torch.zeros(self.C, self.dim))
        self.register_buffer('valid', torch.zeros(self.C, dtype=torch.int32))

    def _check(self, t):
        if t.device.type != 'cuda' or self.weight1.device != t.device:
            raise RuntimeError('VMFHead runs on the GPU, the head on the device of its input (no CPU fallback)')

    def project(self, x2d):
        """rows [M, F] float32 -> [M, dim] through the MLP (differentiable)"""
        from .effdet import meta_ops
        self._check(x2d)
        return meta_ops.projection_forward(x2d, [self.weight1, self.weight2])

    def embed(self, levels):
        """levels -> [B, P, dim] float32, differentiable to the levels and the MLP weights (bfloat16 levels are widened exactly)"""
        if torch.is_tensor(levels):
            if levels.dim() != 3 or levels.shape[2] != self.F:
                raise ValueError('a feature tensor must be [B, P, %d]' % self.F)
            x = levels
        else:
            levels = list(levels)
            if not levels or any(not torch.is_tensor(t) or t.dim() != 4 or t.shape[1] != self.F or t.shape[0] != levels[0].shape[0] for t in levels):
                raise ValueError('levels must be [B, %d, h, w] tensors of one batch size' % self.F)
            B = levels[0].shape[0]
            x = torch.cat([t.permute(0, 2, 3, 1).reshape(B, -1, self.F) for t in levels], 1)
        self._check(x)
        if x.dtype not in (torch.float32, torch.bfloat16):
            raise RuntimeError('levels must be float32 or bfloat16')
        B, P = x.shape[0], x.shape[1]
        return self.project(x.float().reshape(B * P, self.F)).view(B, P, self.dim)

    def loss(self, U, cls_targets, update=True):
        """The loss on embeddings U [B, P, dim] (float32, GPU) themselves: what forward() runs after embed()."""
        if not torch.is_tensor(U) or U.dim() != 3 or U.shape[2] != self.dim or U.dtype != torch.float32:
            raise ValueError('U must be a float32 [B, P, %d] tensor' % self.dim)
        self._check(U)
        if U.shape[0] < 1 or U.shape[1] < 1 or U.shape[0] * U.shape[1] * self.A > MAX_ROWS:
            raise ValueError('B >= 1, P >= 1 and B * A * P <= 2^27')
        loss, stats = _VMFLossFn.apply(U, self.log_kappa, cls_targets, self, bool(update))
        out = {k: (stats[i].to(torch.int64) if i < 3 else stats[i]) for i, k in enumerate(STAT_KEYS)}
        return loss, out

    def forward(self, levels, cls_targets, update=True):
        return self.loss(self.embed(levels), cls_targets, update)


class VMFFeatureOOD(_PyramidRows):
    """The vMF scores of a `VMFHead` under the scorer protocol of `DetBenchPredict` (module docstring).  Reads the head's weights,
    log_kappa and prototypes when called, so a head that trains on is scored as it stands."""
    WANTS_CLASS_TOWER = True                  # DetBenchPredict keeps the class tower and passes its views to score()
    KEYS = ('vmf', 'vmf_class', 'vmf_cosine')

    def __init__(self, head):
        if not isinstance(head, VMFHead):
            raise ValueError('VMFFeatureOOD takes a VMFHead')
        self.head = head
        self.F, self.C, self.A = head.F, head.C, head.A

    def _gather(self, levels, anchor_index, count, A):
        """-> (rows [B * K, F] float32 of the selected anchors, B, P, K, (anchor pointer, count pointer, count is int64), keep)"""
        dt, B, P, table, keep = self._table(levels)
        dev = keep[0].device
        if self.head.weight1.device != dev:
            raise RuntimeError('VMFFeatureOOD: the head must live on the device of the features')
        K, ai_ptr, cnt_ptr, cnt64, keep2 = self._rows(B, dev, anchor_index, count, A * P)
        rows = torch.empty(B * K, self.F, dtype=torch.float32, device=dev)
        _lib.check(_lib.load().effdet_vmf_gather(torch.cuda.current_stream(dev).cuda_stream, dt, *table, self.F, A, B, K, ai_ptr, cnt_ptr, cnt64,
                                                 rows.data_ptr()), 'effdet_vmf_gather')
        return rows, B, P, K, (ai_ptr, cnt_ptr, cnt64), keep + keep2

    def _score(self, levels, anchor_index, count, A, want_rows):
        with torch.no_grad():
            rows, B, P, K, sel, keep = self._gather(levels, anchor_index, count, A)
            U = self.head.project(rows).view(B, K, self.head.dim)
            return _score_rows(self.head, U, P, A, K, sel, True, want_rows)

    def score(self, levels, anchor_index, count=None):
        """Scores of the rows anchor_index [B, K] (int64): dict of [B, K] tensors vmf, vmf_cosine (float32), vmf_class (int64); rows at
        or beyond count[b] and anchors outside [0, A * P) hold 0, -1, 0."""
        if anchor_index is None:
            raise ValueError('score() takes an anchor_index; score_cells() scores every cell')
        return self._score(levels, anchor_index, count, self.A, False)[0]

    def score_cells(self, levels):
        """The same keys for every cell, [B, P]."""
        return self._score(levels, None, None, 1, False)[0]

    def embeddings(self, levels, anchor_index=None, count=None):
        """Unit embeddings: [B, K, dim] of the selected anchors (zeros where a row does not count), or [B, P, dim] of every cell.  At a
        dim that `KNNFeatureOOD` accepts as a width they go into its add() / score() as a [B, P, F] feature tensor."""
        if anchor_index is None:
            return self._score(levels, None, None, 1, True)[1]
        return self._score(levels, anchor_index, count, self.A, True)[1]


def _score_rows(head, U, P, A, K, sel, gathered, want_rows):
    """One call of effdet_vmf_score.  U: [B, P, dim], the row of entry (b, j) the cell of its anchor, or with `gathered` [B, K, dim],
    its row j.  sel: (anchor pointer, count pointer, count is int64).  -> (dict of [B, K] tensors, unit rows [B, K, dim] or None)"""
    lib = _lib.load()
    B, dev = U.shape[0], U.device
    part = partition(head.log_kappa, head.dim)
    out = {'vmf': torch.empty(B, K, dtype=torch.float32, device=dev), 'vmf_class': torch.empty(B, K, dtype=torch.int64, device=dev),
           'vmf_cosine': torch.empty(B, K, dtype=torch.float32, device=dev)}
    unit = torch.empty(B, K, head.dim, dtype=torch.float32, device=dev) if want_rows else None
    ws, n = _ws(lib, B * K, head.C, head.dim, dev)
    _lib.check(lib.effdet_vmf_score(torch.cuda.current_stream(dev).cuda_stream, U.data_ptr(), B, P, A, head.dim, K, *sel, int(gathered), head.C,
                                    head.prototypes.data_ptr(), head.valid.data_ptr(), part['kappa'].data_ptr(), part['logz'].data_ptr(),
                                    out['vmf'].data_ptr(), out['vmf_class'].data_ptr(), out['vmf_cosine'].data_ptr(),
                                    None if unit is None else unit.data_ptr(), ws.data_ptr(), n), 'effdet_vmf_score')
    return out, unit


def _score_embeddings(head, U, anchor_index=None, count=None, want_rows=False, gathered_cells=None):
    """The scores on embeddings themselves, without the MLP (for the tests and tools/vmf_bench.py).  U [B, P, dim] float32 (GPU):
    every cell, or the cells of anchor_index [B, K].  gathered_cells = P: U is [B, K, dim], the rows already gathered for
    anchor_index, which then only decides which entries count."""
    if not torch.is_tensor(U) or U.dim() != 3 or U.shape[2] != head.dim or U.dtype != torch.float32:
        raise ValueError('U must be a float32 [B, P, %d] tensor' % head.dim)
    if U.device.type != 'cuda':
        raise RuntimeError('VMFHead scores: U must be a GPU tensor (no CPU fallback)')
    U = U.detach().contiguous()
    B, P = U.shape[0], (U.shape[1] if gathered_cells is None else int(gathered_cells))
    A = head.A if anchor_index is not None else 1
    K, ai_ptr, cnt_ptr, cnt64, keep = VMFFeatureOOD(head)._rows(B, U.device, anchor_index, count, A * P)
    return _score_rows(head, U, P, A, K, (ai_ptr, cnt_ptr, cnt64), gathered_cells is not None, want_rows)
