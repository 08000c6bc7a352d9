"""Activation-shaping OOD scores on the device (csrc/act_shaping.hip): post-hoc scores that rectify or prune the class
head's penultimate activation - the output d of the depthwise 3 x 3 of `class_net.predict` - and recompute the class logits from it:
ReAct (Sun et al. 2021), ASH-P / ASH-B / ASH-S (Djurisic et al. 2023), SCALE (Xu et al. 2024), DICE weight sparsification (Sun & Li
2022) and GradNorm (Huang et al. 2021).

    model.keep_class_tower = True                                 # the engine keeps the class tower's output (the input of predict)
    s = ActivationShapingOOD(config.fpn_channels, config.num_classes, num_anchors, method='react', percentile=90.0)
    s.set_head(model.class_net)
    s.add_detections(model._engine.class_tower_views(), bench.last_ood['anchor_index'], bench.last_count)   # in-distribution batches
    s.fit()
    bench = DetBenchPredict(model, feature_ood=[s])           # last_ood gains react_energy, react_max_logit, react_class

`add*` accumulate n, sum d (float64, one fixed order) and a 65536-bin histogram of the upper 16 bits of the ordered bit pattern of
every d_j on the device (no host synchronisation, capturable in a graph); `fit` reads them back once: ReAct's threshold c is the
upper edge of the histogram bin that holds the percentile (at or above the exact quantile, relative resolution 2^-7), DICE keeps
the weights whose mean contribution W * mean(d) lies above its p-th percentile.  `score` re-runs the head at selected anchors, one
wave a row; `score_anchors` scores every anchor of every cell, the shaped row formed once per cell and multiplied on the float32-
input MFMA.  The depthwise output is signed, so the ASH / SCALE sums take positive parts (for nonnegative activations these are the
papers' definitions).  `<name>_energy` has the sign of the head's own `energy`; a higher `gradnorm` means more in-distribution.
There is no CPU fallback."""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from .ood_features import MAX_CLASSES, WIDTHS, _PyramidRows, _arr

METHODS = ('none', 'react', 'ash_p', 'ash_b', 'ash_s', 'scale')
HIST_BINS = 65536


def kept_entries(F, percentile):
    """k of the ASH forms and SCALE: F - round(F * percentile / 100) (Python's round); it must lie in [1, F]"""
    k = int(F) - int(round(F * float(percentile) / 100.0))
    if not 1 <= k <= F:
        raise ValueError('percentile %r keeps %d of %d entries: k must lie in [1, F]' % (percentile, k, F))
    return k


def react_threshold(hist, n, F, percentile):
    """The largest finite float32 whose ordered key (bits ^ 2^31 for a cleared sign bit, ~bits otherwise) falls into the first of the
    65536 bins (the key's upper 16 bits) at which the cumulative count reaches ceil(percentile / 100 * n * F), at least 1: at or above
    the exact quantile and within one bin of it.  float64 / integer numpy, reproducible exactly."""
    hist = np.asarray(hist, np.int64)
    if n < 1 or int(hist.sum()) != n * F:
        raise ValueError('the histogram holds %d values, not n * F = %d * %d (n >= 1)' % (int(hist.sum()), n, F))
    target = max(int(math.ceil(float(percentile) / 100.0 * (n * F))), 1)
    b = int(np.searchsorted(np.cumsum(hist), target, side='left'))
    key = np.uint32((b << 16) | 0xFFFF)
    bits = (key ^ np.uint32(0x80000000)) if key & np.uint32(0x80000000) else ~key
    c = np.asarray(bits, np.uint32).reshape(1).view(np.float32)[0]
    if not np.isfinite(c):
        raise ValueError('bin %d holds no finite float32' % b)
    return np.float32(c)


def dice_weight(W, sum_d, n, p):
    """W [A * C, F] float32 -> W with the entries whose mean contribution V = W * (sum_d / n) lies at or below the p-th percentile of
    V (numpy `percentile`, default interpolation, float64, over all A * C rows) set to 0"""
    V = np.asarray(W, np.float32).astype(np.float64) * (np.asarray(sum_d, np.float64) / float(n))[None, :]
    return np.where(V > np.percentile(V, float(p)), np.asarray(W, np.float32), np.float32(0))


def pack_head(W, bias, A):
    """W [A * C, F], bias [A * C] float32 -> (w_rows [A][F][Cp], w_tiles [A][Cp][Fp], bias [A][Cp]) float32 numpy: zero in the
    padding of the weights, -inf in that of the bias (Cp, Fp: C, F rounded up to 16)"""
    W, bias = np.asarray(W, np.float32), np.asarray(bias, np.float32)
    C, F = W.shape[0] // A, W.shape[1]
    Cp, Fp = (C + 15) // 16 * 16, (F + 15) // 16 * 16
    Wr = W.reshape(A, C, F)
    rows, tiles = np.zeros((A, F, Cp), np.float32), np.zeros((A, Cp, Fp), np.float32)
    rows[:, :, :C] = Wr.transpose(0, 2, 1)
    tiles[:, :C, :F] = Wr
    b = np.full((A, Cp), -np.inf, np.float32)
    b[:, :C] = bias.reshape(A, C)
    return rows, tiles, b


class ActivationShapingOOD(_PyramidRows):
    """One shaping method over the class head (module docstring).  num_features: the head width (64, 88, 112, 160, 224 or 288);
    num_classes <= 1024; num_anchors: anchors per cell (A): anchor n sits on cell n // A and uses the weight rows of slot n % A.
    method: none | react | ash_p | ash_b | ash_s | scale; percentile: ReAct's quantile of d, or the share the ASH forms and SCALE
    leave out (k = F - round(F * percentile / 100) entries are kept); dice: None or the percentile of weight contributions to zero;
    gradnorm: also emit `gradnorm` from the unshaped row.  `tower`: the per-level [B, F, h, w] list `Engine.class_tower_views()` or
    `TrainEngine.class_penultimate(tower=True)` returns (channel stride 1; other layouts are copied channels-last)."""
    WANTS_CLASS_TOWER = True                  # DetBenchPredict keeps the class tower and passes its views to score()

    def __init__(self, num_features, num_classes, num_anchors, method='react', percentile=90.0, dice=None, temperature=1.0,
                 gradnorm=False, name=None, device='cuda'):
        self.F, self.C, self.A = int(num_features), int(num_classes), int(num_anchors)
        if self.F not in WIDTHS:
            raise ValueError('num_features must be one of %r, got %d' % (WIDTHS, self.F))
        if not 1 <= self.C <= MAX_CLASSES:
            raise ValueError('num_classes must lie in [1, %d], got %d' % (MAX_CLASSES, self.C))
        if self.A < 1:
            raise ValueError('num_anchors must be >= 1')
        if method not in METHODS:
            raise ValueError('method must be one of %r, got %r' % (METHODS, method))
        self.method, self.percentile = method, float(percentile)
        if not 0.0 <= self.percentile <= 100.0:
            raise ValueError('percentile must lie in [0, 100], got %r' % (percentile,))
        self.k = kept_entries(self.F, self.percentile) if method in METHODS[2:] else 0
        self.dice = None if dice is None else float(dice)
        if self.dice is not None and not 0.0 <= self.dice < 100.0:
            raise ValueError('dice must lie in [0, 100), got %r' % (dice,))
        self.temperature = float(temperature)
        if not (0.0 < self.temperature < float('inf')):
            raise ValueError('temperature must be positive and finite, got %r' % (temperature,))
        self.gradnorm = bool(gradnorm)
        self.name = name if name is not None else method + ('_dice' if self.dice is not None else '')
        self.KEYS = tuple('%s_%s' % (self.name, k) for k in ('energy', 'max_logit', 'class')) + (('gradnorm',) if self.gradnorm else ())
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('ActivationShapingOOD runs on the GPU (no CPU fallback)')
        self.c = None                        # ReAct's threshold (float), set by fit()
        self.fitted = False
        self._head = None                    # float32 numpy (taps [9, F], W [A * C, F], bias [A * C]) of set_head()
        self._dev = None                     # (taps, w_rows, w_tiles, bias) uploads
        self._c_dev = None
        self._stats = None

    needs_fit = property(lambda self: self.method == 'react' or self.dice is not None)

    # ---- head ------------------------------------------------------------------------------------------------------------
    def set_head(self, class_net):
        """Take float32 copies of `class_net.predict`'s depthwise taps, pointwise weight and bias and pack them for the kernels.
        Parameter updates need a new call (a DICE mask is re-applied when a fit exists)."""
        if not hasattr(class_net, 'conv_rep') or not hasattr(class_net, 'predict'):
            raise ValueError('set_head: %s has no conv_rep / predict (a MetaHead keeps its weights elsewhere)' % type(class_net).__name__)
        p = class_net.predict
        taps = p.conv_dw.weight.detach().float().cpu().numpy()
        W = p.conv_pw.weight.detach().float().cpu().numpy()
        if p.conv_pw.bias is None:
            bias = np.zeros(W.shape[0], np.float32)
        else:
            bias = p.conv_pw.bias.detach().float().cpu().numpy()
        if taps.shape != (self.F, 1, 3, 3) or W.shape[:2] != (self.A * self.C, self.F) or W.size != self.A * self.C * self.F:
            raise ValueError('set_head: predict is %r -> %r, expected a 3 x 3 depthwise over %d channels and %d x %d outputs'
                             % (tuple(taps.shape), tuple(W.shape), self.F, self.A, self.C))
        self.set_weights(taps.reshape(self.F, 9).T, W.reshape(self.A * self.C, self.F), bias)
        return self

    def set_weights(self, taps, W, bias):
        """The same from arrays: taps [9, F] (k = 3 ky + kx), W [A * C, F], bias [A * C]."""
        taps, W, bias = (np.ascontiguousarray(np.asarray(t, np.float32)) for t in (taps, W, bias))
        if taps.shape != (9, self.F) or W.shape != (self.A * self.C, self.F) or bias.shape != (self.A * self.C,):
            raise ValueError('set_weights: taps [9, %d], W [%d, %d], bias [%d]' % (self.F, self.A * self.C, self.F, self.A * self.C))
        self._head = (taps, W, bias)
        self._upload(W if not (self.fitted and self.dice is not None) else self._masked())
        return self

    def _masked(self):
        n, sum_d, _ = (t.cpu().numpy() for t in self._setup())
        return dice_weight(self._head[1], sum_d, int(n[0]), self.dice)

    def _upload(self, W):
        taps, _, bias = self._head
        self.weight = W                      # the float32 weight the scores use (DICE-masked after a fit)
        self._dev = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(self.device) for a in (taps,) + pack_head(W, bias, self.A))

    # ---- storage ---------------------------------------------------------------------------------------------------------
    def _setup(self):
        if self._stats is None:
            dev = self.device
            self._stats = (torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(self.F, dtype=torch.float64, device=dev),
                           torch.zeros(HIST_BINS, dtype=torch.int64, device=dev))
        return self._stats

    n = property(lambda self: self._setup()[0])
    sum_d = property(lambda self: self._setup()[1])
    hist = property(lambda self: self._setup()[2])

    def _tower(self, tower):
        """tower -> (dtype code, B, P, the level table with heights and widths, tensors to keep alive)"""
        if torch.is_tensor(tower):
            raise ValueError('tower must be the per-level list of [B, %d, h, w] tensors' % self.F)
        dt, B, P, table, keep = self._table(tower)
        hw = (_arr([int(t.shape[2]) for t in keep], ctypes.c_int), _arr([int(t.shape[3]) for t in keep], ctypes.c_int))
        return dt, B, P, table + hw, keep

    def _need_head(self):
        if self._dev is None:
            raise RuntimeError('ActivationShapingOOD: set_head() comes first')

    # ---- fit -------------------------------------------------------------------------------------------------------------
    def clear(self):
        """Forget every row and the fit (a device-side reset, no synchronisation)."""
        for t in self._setup():
            t.zero_()
        self._unfit()

    def _unfit(self):
        self.c, self._c_dev, was = None, None, self.fitted
        self.fitted = False
        if was and self.dice is not None and self._head is not None:
            self._upload(self._head[1])

    def add(self, tower, anchor_index=None, count=None):
        """Add rows to the statistics: row (b, j) is the cell of anchor anchor_index[b, j] (int64 [B, K]; None: anchor j, K = A * P);
        it counts when j < count[b] (None: all).  Rows with a non-finite d_j are skipped."""
        self._need_head()
        dt, B, P, table, keep = self._tower(tower)
        dev = keep[0].device
        K, ai_ptr, cnt_ptr, cnt64, keep2 = self._rows(B, dev, anchor_index, count, self.A * P)
        n, sum_d, hist = self._setup()
        lib = _lib.load()
        st, ws = self._stream_ws(dev, lib.effdet_act_shaping_workspace_bytes(B * K, self.F), B * K)
        _lib.check(lib.effdet_act_shaping_fit(st, dt, *table, self.F, self.A, B, K, ai_ptr, cnt_ptr, cnt64, self._dev[0].data_ptr(),
                                              n.data_ptr(), sum_d.data_ptr(), hist.data_ptr(), ws.data_ptr(), ws.numel()),
                   'effdet_act_shaping_fit')

    def add_detections(self, tower, anchor_index, count):
        """Add the kept detections of a `DetBenchPredict` pass: anchor_index = bench.last_ood['anchor_index'], count = bench.last_count."""
        if anchor_index is None:
            raise ValueError('add_detections() takes an anchor_index')
        self.add(tower, anchor_index, count)

    def add_targets(self, tower, cls_targets):
        """Add every anchor with a class >= 0 of the per-level [B, H, W, A] label maps of `AnchorLabeler` (positive anchors only)."""
        B = cls_targets[0].shape[0]
        labels = torch.cat([t.reshape(B, -1) for t in cls_targets], 1)
        pos = labels >= 0
        order = torch.sort((~pos).to(torch.int8), dim=1, stable=True)[1]          # the positive anchors first, ascending
        self.add(tower, order.to(torch.int64), pos.sum(1).to(torch.int64))

    def fit(self):
        """Statistics -> ReAct's threshold and the DICE mask (float64 host glue; one device-to-host read of n, sum_d and hist)."""
        self._need_head()
        packed = torch.cat([self.n.double(), self.sum_d, self.hist.double()]).cpu().numpy()           # (counts < 2^53: exact)
        n, sum_d, hist = int(packed[0]), packed[1:1 + self.F], packed[1 + self.F:].astype(np.int64)
        if self.needs_fit and n < 1:
            raise ValueError('ActivationShapingOOD.fit: no rows were added')
        if self.method == 'react':
            self.c = float(react_threshold(hist, n, self.F, self.percentile))
            self._c_dev = torch.tensor([self.c], dtype=torch.float32, device=self.device)
        self.fitted = True
        if self.dice is not None:
            self._upload(dice_weight(self._head[1], sum_d, n, self.dice))
        return self

    # ---- score -----------------------------------------------------------------------------------------------------------
    def _ready(self):
        self._need_head()
        if self.needs_fit and not self.fitted:
            raise RuntimeError('ActivationShapingOOD(%s): fit() comes before score()' % self.name)

    def _outputs(self, B, K, dev):
        f = [torch.empty(B, K, dtype=torch.float32, device=dev) for _ in range(3 if self.gradnorm else 2)]
        cls = torch.empty(B, K, dtype=torch.int64, device=dev)
        out = {self.KEYS[0]: f[0], self.KEYS[1]: f[1], self.KEYS[2]: cls}
        if self.gradnorm:
            out['gradnorm'] = f[2]
        return out, (f[0].data_ptr(), f[1].data_ptr(), cls.data_ptr(), f[2].data_ptr() if self.gradnorm else None)

    def _method_args(self):
        return (METHODS.index(self.method), self.k, None if self._c_dev is None else self._c_dev.data_ptr(), self.temperature)

    def score(self, tower, anchor_index, count=None, rows=False):
        """Scores of the rows anchor_index [B, K] (int64): dict of [B, K] tensors - `<name>_energy`, `<name>_max_logit` float32,
        `<name>_class` int64, `gradnorm` when requested - and with rows=True `rows` [B, K, F] float32, the shaped activations x';
        rows at or beyond count[b] hold 0, 0, -1 (and zeros)."""
        self._ready()
        if anchor_index is None:
            raise ValueError('score() takes an anchor_index; score_anchors() scores every anchor')
        dt, B, P, table, keep = self._tower(tower)
        dev = keep[0].device
        K, ai_ptr, cnt_ptr, cnt64, keep2 = self._rows(B, dev, anchor_index, count, self.A * P)
        out, ptrs = self._outputs(B, K, dev)
        xr = torch.empty(B, K, self.F, dtype=torch.float32, device=dev) if rows else None
        taps, w_rows, _, bias = self._dev
        st, _ = self._stream_ws(dev)
        _lib.check(_lib.load().effdet_act_shaping_score(st, dt, *table, self.F, self.C, self.A, B, K, ai_ptr, cnt_ptr, cnt64, taps.data_ptr(),
                                                        w_rows.data_ptr(), bias.data_ptr(), *self._method_args(), *ptrs,
                                                        None if xr is None else xr.data_ptr()), 'effdet_act_shaping_score')
        if rows:
            out['rows'] = xr
        return out

    def score_anchors(self, tower):
        """The same keys for every anchor of every cell, [B, N] with N = A * P in the head's anchor order (cell * A + slot)."""
        self._ready()
        dt, B, P, table, keep = self._tower(tower)
        dev = keep[0].device
        out, ptrs = self._outputs(B, self.A * P, dev)
        taps, _, w_tiles, bias = self._dev
        st, _ = self._stream_ws(dev)
        _lib.check(_lib.load().effdet_act_shaping_score_cells(st, dt, *table, self.F, self.C, self.A, B, taps.data_ptr(), w_tiles.data_ptr(),
                                                              bias.data_ptr(), *self._method_args(), *ptrs), 'effdet_act_shaping_score_cells')
        return out

    # ---- state -----------------------------------------------------------------------------------------------------------
    def _geometry(self):
        return {'num_features': self.F, 'num_classes': self.C, 'num_anchors': self.A, 'method': self.method, 'percentile': self.percentile,
                'dice': self.dice}

    def state_dict(self):
        n, sum_d, hist = self._setup()
        return dict(self._geometry(), temperature=self.temperature, n=n.cpu(), sum_d=sum_d.cpu(), hist=hist.cpu(), fitted=self.fitted, c=self.c)

    def _check_geometry(self, d, what):
        for key, mine in self._geometry().items():
            if d[key] != mine:
                raise ValueError('%s: %s differs (%r, %r)' % (what, key, d[key], mine))

    def load_state_dict(self, d):
        """Statistics and the fitted values travel: the threshold c as stored, the DICE mask re-derived from the statistics."""
        self._check_geometry(d, 'load_state_dict')
        self._unfit()
        for dst, k in zip(self._setup(), ('n', 'sum_d', 'hist')):
            dst.copy_(torch.as_tensor(d[k]).to(dst.dtype).reshape(dst.shape))
        self.temperature = float(d.get('temperature', self.temperature))
        if d.get('fitted'):
            if self.dice is not None:
                self._need_head()
                self._upload(self._masked())
            if self.method == 'react':
                self.c = float(d['c'])
                self._c_dev = torch.tensor([self.c], dtype=torch.float32, device=self.device)
            self.fitted = True
        return self

    def merge_(self, other):
        """Add the statistics of another ActivationShapingOOD (or of its state dict), e.g. another rank's; fit() again afterwards."""
        od = other.state_dict() if isinstance(other, ActivationShapingOOD) else other
        self._check_geometry(od, 'merge_')
        for dst, k in zip(self._setup(), ('n', 'sum_d', 'hist')):
            dst.add_(torch.as_tensor(od[k]).to(device=self.device, dtype=dst.dtype).reshape(dst.shape))
        self._unfit()
        return self
