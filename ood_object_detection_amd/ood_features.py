"""Feature-space OOD scores on the device (csrc/feature_ood.hip): the class-conditional Gaussian (Mahalanobis)
distance with a tied covariance, and its relative form, over rows of the BiFPN pyramid.

    f = FeatureOOD(config.fpn_channels, config.num_classes, num_anchors)
    f.add_detections(model(x, mode='fpn')[1], det, bench.last_ood['anchor_index'], bench.last_count)    # in-distribution batches
    f.fit()
    bench = DetBenchPredict(model, feature_ood=f)           # last_ood gains mahalanobis, relative_mahalanobis, nearest_class

`add*` accumulate n_c, s_c = sum f and S = sum f f^T in float64 on the device (no host synchronisation, capturable in a graph,
bit-identical from run to run); `fit` reads the (C + F) * F + C numbers back once and forms the whitening factors in float64
with numpy; `score*` run three float32 products per row on the float32-input MFMA.  A higher score means more in-distribution,
so both feed `ood.OODEvaluator` unchanged.  There is no CPU fallback.

`KNNFeatureOOD` (csrc/feature_knn.hip) is the non-parametric counterpart: a bank of in-distribution rows and minus the squared
distance to the k-th nearest of them ("deep nearest neighbours", Sun et al. 2022), with the same `add*` / `fit` / `score*` calls:

    f = KNNFeatureOOD(config.fpn_channels, num_anchors, capacity=1 << 18, k=10, num_classes=config.num_classes)
    f.add_detections(levels, det, bench.last_ood['anchor_index'], bench.last_count)
    f.fit()
    bench = DetBenchPredict(model, feature_ood=[maha, f])   # last_ood gains knn, knn_index, knn_class as well"""
import ctypes

import numpy as np
import torch

from . import _lib

WIDTHS = (64, 88, 112, 160, 224, 288)         # every BiFPN width the engine builds (d0 .. d5)
MAX_CLASSES = 1024
MAX_LEVELS = 8
MAX_ROWS = 1 << 27


def finalize(n_c, s_c, S, shrinkage=0.0):
    """Statistics -> scoring parameters, float64 numpy (parameter-sized host glue, once per fit).
    Returns dict(mu [C, F], mu0 [F], cov, cov0 [F, F], W, W0 [F, F] (inverse Cholesky factors), M [C, F] = W (mu_c - mu_0),
    m2 [C] = |M_c|^2 (+inf for a class without rows), n).  shrinkage: cov <- cov + shrinkage * (tr cov / F) * I, both covariances."""
    n_c = np.asarray(n_c, np.int64)
    s_c, S = np.asarray(s_c, np.float64), np.asarray(S, np.float64)
    C, F = s_c.shape
    n = int(n_c.sum())
    if n < 1:
        raise ValueError('FeatureOOD.fit: no rows were added')
    if not (float(shrinkage) >= 0.0):
        raise ValueError('shrinkage must be >= 0')
    have = n_c > 0
    mu = np.zeros((C, F))
    mu[have] = s_c[have] / n_c[have, None]
    cov = (S - (mu * n_c[:, None].astype(np.float64)).T @ mu) / n
    mu0 = s_c.sum(0) / n
    cov0 = S / n - np.outer(mu0, mu0)
    remedy = 'add more rows than F = %d (beyond one per class), or pass fit(shrinkage=...) > 0' % F
    if shrinkage == 0.0 and n - int(have.sum()) < F:
        raise ValueError('FeatureOOD.fit: %d rows of %d classes give a singular tied covariance: %s' % (n, int(have.sum()), remedy))
    factors = []
    for m in (cov, cov0):
        m = 0.5 * (m + m.T)
        if shrinkage:
            m = m + float(shrinkage) * (np.trace(m) / F) * np.eye(F)
        try:
            L = np.linalg.cholesky(m)
        except np.linalg.LinAlgError:
            L = None
        if L is None or not np.isfinite(L).all() or L.diagonal().min() <= 1e-7 * np.sqrt(max(np.trace(m), 0.0) / F):
            raise ValueError('FeatureOOD.fit: the covariance is singular (Cholesky failed): ' + remedy)
        factors.append((m, L, np.linalg.solve(L, np.eye(F))))
    (cov, _, W), (cov0, _, W0) = factors
    M = (mu - mu0) @ W.T
    M[~have] = 0.0
    m2 = np.where(have, (M * M).sum(1), np.inf)
    return {'mu': mu, 'mu0': mu0, 'cov': cov, 'cov0': cov0, 'W': W, 'W0': W0, 'M': M, 'm2': m2, 'n': n}


def merged_state(a, b):
    """The state dict of the union of two sets of rows (the statistics are additive); the fit is not carried over."""
    for k in ('num_features', 'num_classes', 'num_anchors'):
        if a[k] != b[k]:
            raise ValueError('merge: %s differs (%r, %r)' % (k, a[k], b[k]))
    out = {k: a[k] for k in ('num_features', 'num_classes', 'num_anchors')}
    for k in ('n_c', 's_c', 'S'):
        out[k] = a[k] + b[k]
    return out


def anchor_cells(anchor_index, level_hw, num_anchors):
    """The kernels' addressing restated (numpy): anchor n of the head outputs [B, N, C], N = A * P, sits on cell n // A of the
    packed pyramid; the level follows from the cumulative cell counts.  -> (level, y, x) int64 arrays."""
    n = np.asarray(anchor_index, np.int64)
    cell = n // int(num_anchors)
    starts = np.concatenate([[0], np.cumsum([h * w for h, w in level_hw])])
    if n.size and (n.min() < 0 or cell.max() >= starts[-1]):
        raise ValueError('anchor index outside [0, A * P)')
    level = np.searchsorted(starts, cell, side='right') - 1
    local = cell - starts[level]
    widths = np.asarray([w for _, w in level_hw], np.int64)[level]
    return level, local // widths, local % widths


def _arr(values, ctype):
    return (ctype * len(values))(*values)


class _PyramidRows:
    """Row addressing shared by the feature-space scorers: the level table and the anchor_index / count arguments of a call."""

    def _table(self, levels):
        """levels -> (dtype code, B, P, ctypes arrays of the level table, tensors to keep alive)"""
        if torch.is_tensor(levels):
            if levels.dim() != 3:
                raise ValueError('a feature tensor must be [B, P, F]')
            views = [levels.unsqueeze(2).permute(0, 3, 1, 2)]                      # [B, F, P, 1]
        else:
            views = list(levels)
        if not 1 <= len(views) <= MAX_LEVELS:
            raise ValueError('between 1 and %d levels' % MAX_LEVELS)
        keep, rows = [], []
        for t in views:
            if not torch.is_tensor(t) or t.device.type != 'cuda':
                raise RuntimeError('%s: features must be GPU tensors (no CPU fallback)' % type(self).__name__)
            if t.dim() != 4 or t.shape[1] != self.F or t.shape[0] != views[0].shape[0] or t.dtype != views[0].dtype or t.device != views[0].device:
                raise ValueError('levels must be [B, %d, H, W] tensors of one batch size, dtype and device' % self.F)
            if t.dtype not in (torch.float32, torch.bfloat16):
                raise RuntimeError('features must be float32 or bfloat16')
            t = t.detach()
            H, W = t.shape[2], t.shape[3]
            if t.stride(1) != 1 or min(t.stride()) < 0 or (H > 1 and W > 1 and t.stride(2) != W * t.stride(3)):
                t = t.contiguous(memory_format=torch.channels_last)
            cell = t.stride(3) if W > 1 else (t.stride(2) if H > 1 else self.F)
            keep.append(t)
            rows.append((t.data_ptr(), H * W, t.stride(0), cell, 1))
        B, P = views[0].shape[0], sum(r[1] for r in rows)
        if B < 1 or B * P > 1 << 31:
            raise ValueError('B * P must lie in [1, 2^31]')
        table = (len(rows), _arr([r[0] for r in rows], ctypes.c_void_p)) + tuple(_arr([r[k] for r in rows], ctypes.c_longlong) for k in (1, 2, 3, 4))
        return (0 if views[0].dtype == torch.float32 else 1), B, P, table, keep

    def _rows(self, B, dev, anchor_index, count, K):
        """anchor_index / count -> (K, pointers, tensors to keep alive)"""
        keep = []
        ai_ptr = None
        if anchor_index is not None:
            if anchor_index.device != dev or anchor_index.dim() != 2 or anchor_index.shape[0] != B or anchor_index.dtype != torch.int64:
                raise ValueError('anchor_index: an int64 [B, K] tensor on the device of the features')
            anchor_index = anchor_index.detach().contiguous()
            keep.append(anchor_index)
            ai_ptr, K = anchor_index.data_ptr(), anchor_index.shape[1]
        cnt_ptr, cnt64 = None, 0
        if count is not None:
            if count.device != dev or count.dtype not in (torch.int32, torch.int64) or count.numel() != B:
                raise ValueError('count: an int32 or int64 tensor of B entries on the device of the features')
            count = count.detach().reshape(B).contiguous()
            keep.append(count)
            cnt_ptr, cnt64 = count.data_ptr(), int(count.dtype == torch.int64)
        if K < 1 or B * K > MAX_ROWS:
            raise ValueError('between 1 and 2^27 rows per call')
        return K, ai_ptr, cnt_ptr, cnt64, keep


class FeatureOOD(_PyramidRows):
    """Running class statistics of pyramid features and the two scores that follow from them (module docstring).
    num_features: the BiFPN width (64, 88, 112, 160, 224 or 288); num_classes <= 1024; num_anchors: anchors per cell (A), so
    that anchor n sits on cell n // A."""
    KEYS = ('mahalanobis', 'relative_mahalanobis', 'nearest_class')       # of the dict score() returns

    def __init__(self, num_features, num_classes, num_anchors, device='cuda'):
        self.F, self.C, self.A = int(num_features), int(num_classes), int(num_anchors)
        if self.F not in WIDTHS:
            raise ValueError('num_features must be one of %r, got %d' % (WIDTHS, self.F))
        if not 1 <= self.C <= MAX_CLASSES:
            raise ValueError('num_classes must lie in [1, %d], got %d' % (MAX_CLASSES, self.C))
        if self.A < 1:
            raise ValueError('num_anchors must be >= 1')
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('FeatureOOD runs on the GPU (no CPU fallback)')
        self.shrinkage = None                # set by fit()
        self.params = None                   # float64 numpy results of the last fit (finalize())
        self._dev = None                     # their padded float32 uploads
        self._stats = None
        self._ws = None

    # ---- storage ---------------------------------------------------------------------------------------------------------
    def _setup(self):
        if self._stats is None:
            dev = self.device
            self._stats = (torch.zeros(self.C, dtype=torch.int64, device=dev), torch.zeros(self.C, self.F, dtype=torch.float64, device=dev),
                           torch.zeros(self.F, self.F, dtype=torch.float64, device=dev))
        return self._stats

    n_c = property(lambda self: self._setup()[0])
    s_c = property(lambda self: self._setup()[1])
    S = property(lambda self: self._setup()[2])

    def _workspace(self, rows):
        need = _lib.load().effdet_feature_ood_workspace_bytes(rows, self.F)
        if need <= 0:
            raise ValueError('between 1 and 2^27 rows per call, got %d' % rows)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    # ---- fit -------------------------------------------------------------------------------------------------------------
    def clear(self):
        """Forget every row and the fit (a device-side reset, no synchronisation)."""
        for t in self._setup():
            t.zero_()
        self.shrinkage = self.params = self._dev = None

    def add(self, levels, classes, anchor_index=None, count=None, class_offset=0):
        """Add rows.  levels: the list `model(x, mode='fpn')[1]` / `mode='supp_bb'` returns ([B, F, H, W] per level; a level
        whose channel stride is not 1 is copied channels-last) or one [B, P, F] tensor.  Row (b, j) is the feature of the cell
        of anchor anchor_index[b, j] (int64 [B, K]; None: anchor j, the dense form with K = A * P) with class
        classes[b, j] - class_offset (int32, int64 or float32 [B, K], strided views are fine); it counts when j < count[b]
        (None: all) and the class lies in [0, num_classes) - so -1 / ignore labels pass through."""
        dt, B, P, table, keep = self._table(levels)
        dev = keep[0].device
        if not torch.is_tensor(classes) or classes.device != dev or classes.dim() != 2 or classes.shape[0] != B:
            raise ValueError('classes: a [B, K] tensor on the device of the features')
        if classes.dtype not in (torch.int32, torch.int64, torch.float32):
            raise ValueError('classes must be int32, int64 or float32')
        K, ai_ptr, cnt_ptr, cnt64, keep2 = self._rows(B, dev, anchor_index, count, self.A * P)
        if classes.shape[1] != K:
            raise ValueError('classes must be [B, %d] like the rows' % K)
        classes = classes.detach()
        if min(classes.stride()) < 0:
            classes = classes.contiguous()
        cdt = {torch.int32: 0, torch.int64: 1, torch.float32: 2}[classes.dtype]
        n_c, s_c, S = self._setup()
        ws = self._workspace(B * K)
        lib = _lib.load()
        st = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(lib.effdet_feature_ood_fit(st, dt, *table, self.F, self.C, self.A, B, K, ai_ptr, classes.data_ptr(), cdt,
                                              classes.stride(0), classes.stride(1), int(class_offset), cnt_ptr, cnt64,
                                              n_c.data_ptr(), s_c.data_ptr(), S.data_ptr(), ws.data_ptr(), ws.numel()),
                   'effdet_feature_ood_fit')

    def add_detections(self, levels, det, anchor_index, count):
        """Add the kept detections of a `DetBenchPredict` pass: det [B, max_det, 6] (class + 1 in det[..., 5]),
        anchor_index = bench.last_ood['anchor_index'], count = bench.last_count."""
        if not torch.is_tensor(det) or det.dim() != 3 or det.shape[2] != 6 or det.dtype != torch.float32:
            raise ValueError('det must be a float32 [B, max_det, 6] tensor')
        self.add(levels, det[..., 5], anchor_index, count, class_offset=1)

    def add_targets(self, levels, cls_targets):
        """Add every anchor with a class >= 0 of the per-level [B, H, W, A] label maps of `AnchorLabeler` (the dense form)."""
        B = cls_targets[0].shape[0]
        self.add(levels, torch.cat([t.reshape(B, -1) for t in cls_targets], 1))

    def fit(self, shrinkage=0.0):
        """Statistics -> whitening factors and class means (`finalize`; reads (C + F) * F + C numbers back, synchronises).
        ValueError when a covariance is singular: add more rows than F, or pass a shrinkage."""
        n_c, s_c, S = self._setup()
        p = finalize(n_c.cpu().numpy(), s_c.cpu().numpy(), S.cpu().numpy(), shrinkage)
        F, C = self.F, self.C
        Fp, Cp = (F + 15) // 16 * 16, (C + 31) // 32 * 32
        W, W0, M = np.zeros((Fp, Fp), np.float32), np.zeros((Fp, Fp), np.float32), np.zeros((Cp, Fp), np.float32)
        m2, mu0 = np.full(Cp, np.inf, np.float32), np.zeros(Fp, np.float32)
        W[:F, :F], W0[:F, :F], M[:C, :F], m2[:C], mu0[:F] = p['W'], p['W0'], p['M'], p['m2'], p['mu0']
        self._dev = tuple(torch.from_numpy(a).to(self.device) for a in (W, W0, M, m2, mu0))
        self.params, self.shrinkage = p, float(shrinkage)
        return self

    # ---- score -----------------------------------------------------------------------------------------------------------
    def _score(self, levels, anchor_index, count, A):
        if self._dev is None:
            raise RuntimeError('FeatureOOD: fit() comes before score()')
        dt, B, P, table, keep = self._table(levels)
        dev = keep[0].device
        K, ai_ptr, cnt_ptr, cnt64, keep2 = self._rows(B, dev, anchor_index, count, A * P)
        maha = torch.empty(B, K, dtype=torch.float32, device=dev)
        rel = torch.empty_like(maha)
        near = torch.empty(B, K, dtype=torch.int32, device=dev)
        lib = _lib.load()
        st = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(lib.effdet_feature_ood_score(st, dt, *table, self.F, self.C, A, B, K, ai_ptr, cnt_ptr, cnt64,
                                                *[t.data_ptr() for t in self._dev], maha.data_ptr(), rel.data_ptr(), near.data_ptr()),
                   'effdet_feature_ood_score')
        return {'mahalanobis': maha, 'relative_mahalanobis': rel, 'nearest_class': near}

    def score(self, levels, anchor_index, count=None):
        """Scores of the rows anchor_index [B, K] (int64): dict(mahalanobis, relative_mahalanobis [B, K] float32, nearest_class
        [B, K] int32); rows at or beyond count[b] hold 0, 0, -1 like the zero-padded detections."""
        if anchor_index is None:
            raise ValueError('score() takes an anchor_index; score_cells() scores every cell')
        return self._score(levels, anchor_index, count, self.A)

    def score_cells(self, levels):
        """The same keys for every cell of the pyramid, [B, P]."""
        return self._score(levels, None, None, 1)

    # ---- state -----------------------------------------------------------------------------------------------------------
    def state_dict(self):
        n_c, s_c, S = self._setup()
        d = {'num_features': self.F, 'num_classes': self.C, 'num_anchors': self.A, 'n_c': n_c.cpu(), 's_c': s_c.cpu(), 'S': S.cpu()}
        if self.shrinkage is not None:
            d['shrinkage'] = self.shrinkage
        return d

    def load_state_dict(self, d):
        if (d['num_features'], d['num_classes'], d['num_anchors']) != (self.F, self.C, self.A):
            raise ValueError('state dict of another geometry')
        for dst, k in zip(self._setup(), ('n_c', 's_c', 'S')):
            dst.copy_(torch.as_tensor(d[k]).to(dst.dtype))
        self.shrinkage = self.params = self._dev = None
        if d.get('shrinkage') is not None:
            self.fit(d['shrinkage'])
        return self

    def merge_(self, other):
        """Add the statistics of another FeatureOOD (or of its state dict), e.g. another rank's; fit() again afterwards."""
        od = other.state_dict() if isinstance(other, FeatureOOD) else other
        if (od['num_features'], od['num_classes'], od['num_anchors']) != (self.F, self.C, self.A):
            raise ValueError('merge_: another geometry')
        for dst, k in zip(self._setup(), ('n_c', 's_c', 'S')):
            dst.add_(torch.as_tensor(od[k]).to(device=self.device, dtype=dst.dtype))
        self.shrinkage = self.params = self._dev = None
        return self


class KNNFeatureOOD(_PyramidRows):
    """A bank of in-distribution pyramid rows and the k-nearest-neighbour score against it (csrc/feature_knn.hip).

    `add*` append the valid rows to the bank on the device (no host synchronisation, capturable in a graph): the valid row with
    ordinal g since `clear()` - counted across calls - is kept when g % sample_every == 0, so the bank does not depend on how the
    rows are split into calls; rows beyond `capacity` are dropped and counted in `lost`.  With `normalize` a row r is stored as
    r * (1 / sqrt(max(|r|^2, 1e-24))), and queries are treated alike.  `fit` reads the three counters once and fixes the bank size
    M and k; `score*` return, per row, float32

        knn        = -d2 of the min(k, M)-th nearest bank row,  d2_i = max((|q|^2 + |r_i|^2) - 2 q.r_i, 0)
        knn_index  = the nearest bank row (the lower row on a tie), knn_class = its class (-1 without classes)

    and 0, -1, -1 at or beyond count[b].  The SQUARED distance is emitted, not its root as in Sun et al.: it is monotone in their
    score, so every metric of `ood.OODEvaluator` is the same, and its float32 error is absolute and bounded, which the root's is
    not near zero.  The dot products run on the float32-input MFMA; results are bit-identical from run to run and for every
    `splits`.  num_features: the BiFPN width; capacity <= 2^24 rows; 1 <= k <= 32; num_classes None: rows carry no class and
    `classes` may be None.  There is no CPU fallback."""
    MAX_K, MAX_CAPACITY, MAX_SPLITS = 32, 1 << 24, 64
    KEYS = ('knn', 'knn_index', 'knn_class')

    def __init__(self, num_features, num_anchors, capacity, k=10, num_classes=None, normalize=True, sample_every=1, device='cuda'):
        self.F, self.A = int(num_features), int(num_anchors)
        self.C = 0 if num_classes is None else int(num_classes)
        self.capacity, self.k, self.normalize, self.sample_every = int(capacity), int(k), bool(normalize), int(sample_every)
        if self.F not in WIDTHS:
            raise ValueError('num_features must be one of %r, got %d' % (WIDTHS, self.F))
        if num_classes is not None and self.C < 1:
            raise ValueError('num_classes must be >= 1 or None')
        if self.A < 1:
            raise ValueError('num_anchors must be >= 1')
        if not 1 <= self.capacity <= self.MAX_CAPACITY:
            raise ValueError('capacity must lie in [1, 2^24], got %d' % self.capacity)
        if not 1 <= self.k <= self.MAX_K:
            raise ValueError('k must lie in [1, %d], got %d' % (self.MAX_K, self.k))
        if self.sample_every < 1:
            raise ValueError('sample_every must be >= 1')
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('KNNFeatureOOD runs on the GPU (no CPU fallback)')
        self.Fp = (self.F + 15) // 16 * 16
        self.splits = 0                      # bank parts of a score call; 0: chosen by the library (the results do not depend on it)
        self.M = None                        # bank rows the scores look at, set by fit()
        self._bank = None

    # ---- storage ---------------------------------------------------------------------------------------------------------
    def _setup(self):
        if self._bank is None:
            dev = self.device
            self._bank = (torch.zeros(self.capacity, self.Fp, dtype=torch.float32, device=dev),
                          torch.zeros(self.capacity, dtype=torch.float32, device=dev),
                          torch.zeros(self.capacity, dtype=torch.int32, device=dev), torch.zeros(3, dtype=torch.int64, device=dev))
        return self._bank

    rows = property(lambda self: self._setup()[0])
    norms = property(lambda self: self._setup()[1])
    classes = property(lambda self: self._setup()[2])
    counters = property(lambda self: self._setup()[3])       # size, seen, lost (device, int64)

    def _counts(self):
        return [int(v) for v in self.counters.cpu()]

    size = property(lambda self: self._counts()[0])          # these three synchronise
    seen = property(lambda self: self._counts()[1])
    lost = property(lambda self: self._counts()[2])

    def _workspace(self, rows, k, splits, dev):
        """A workspace of this call's own (the caching allocator hands it out per stream, so the sub-batch streams of a
        `DetBenchPredict` do not share one; inside a graph capture it comes from the graph's pool)."""
        need = _lib.load().effdet_feature_knn_workspace_bytes(rows, self.F, k, splits)
        if need <= 0:
            raise ValueError('between 1 and 2^27 rows per call, got %d' % rows)
        return torch.empty(need, dtype=torch.uint8, device=dev)

    # ---- bank ------------------------------------------------------------------------------------------------------------
    def clear(self):
        """Forget every row and the fit (a device-side reset, no synchronisation)."""
        self.counters.zero_()
        self.M = None

    def add(self, levels, classes=None, anchor_index=None, count=None, class_offset=0):
        """Append rows (arguments as `FeatureOOD.add`).  Without num_classes `classes` may be None; with it, a row whose class
        lies outside [0, num_classes) is skipped."""
        dt, B, P, table, keep = self._table(levels)
        dev = keep[0].device
        K, ai_ptr, cnt_ptr, cnt64, keep2 = self._rows(B, dev, anchor_index, count, self.A * P)
        cls_ptr, cdt, pitch, stride = None, 0, 0, 0
        if self.C:
            if not torch.is_tensor(classes) or classes.device != dev or classes.dim() != 2 or tuple(classes.shape) != (B, K):
                raise ValueError('classes: a [B, %d] tensor on the device of the features' % K)
            if classes.dtype not in (torch.int32, torch.int64, torch.float32):
                raise ValueError('classes must be int32, int64 or float32')
            classes = classes.detach()
            if min(classes.stride()) < 0:
                classes = classes.contiguous()
            cls_ptr, cdt = classes.data_ptr(), {torch.int32: 0, torch.int64: 1, torch.float32: 2}[classes.dtype]
            pitch, stride = classes.stride(0), classes.stride(1)
        bank, norms, bcls, counters = self._setup()
        ws = self._workspace(B * K, 0, 0, dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(_lib.load().effdet_feature_knn_append(st, dt, *table, self.F, self.C, self.A, B, K, ai_ptr, cls_ptr, cdt, pitch, stride,
                                                         int(class_offset), cnt_ptr, cnt64, int(self.normalize), self.sample_every,
                                                         self.capacity, bank.data_ptr(), norms.data_ptr(), bcls.data_ptr(),
                                                         counters.data_ptr(), ws.data_ptr(), ws.numel()), 'effdet_feature_knn_append')
        self.M = None

    def add_detections(self, levels, det, anchor_index, count):
        """Append the kept detections of a `DetBenchPredict` pass: det [B, max_det, 6] (class + 1 in det[..., 5]),
        anchor_index = bench.last_ood['anchor_index'], count = bench.last_count."""
        if not torch.is_tensor(det) or det.dim() != 3 or det.shape[2] != 6 or det.dtype != torch.float32:
            raise ValueError('det must be a float32 [B, max_det, 6] tensor')
        self.add(levels, det[..., 5] if self.C else None, anchor_index, count, class_offset=1)

    def add_targets(self, levels, cls_targets):
        """Append every anchor with a class >= 0 of the per-level [B, H, W, A] label maps of `AnchorLabeler` (the dense form; one
        d0 batch of 64 has about 49 k of them: choose `sample_every`)."""
        B = cls_targets[0].shape[0]
        labels = torch.cat([t.reshape(B, -1) for t in cls_targets], 1)
        if not self.C:
            raise ValueError('add_targets selects rows by their class: construct with num_classes')
        self.add(levels, labels)

    def fit(self, k=None):
        """Fix the bank size M and k for the scores (reads the three counters once: the only synchronisation).  Warns when rows
        were lost to the capacity; ValueError when the bank is empty."""
        if k is not None:
            if not 1 <= int(k) <= self.MAX_K:
                raise ValueError('k must lie in [1, %d], got %d' % (self.MAX_K, int(k)))
            self.k = int(k)
        size, seen, lost = self._counts()
        if lost > 0:
            import warnings
            warnings.warn('KNNFeatureOOD: %d rows beyond the capacity of %d were dropped (raise capacity or sample_every)' % (lost, self.capacity))
        if size < 1:
            raise ValueError('KNNFeatureOOD.fit: no rows were added')
        self.M = size
        return self

    # ---- score -----------------------------------------------------------------------------------------------------------
    def _score(self, levels, anchor_index, count, A):
        if self.M is None:
            raise RuntimeError('KNNFeatureOOD: fit() comes before score()')
        dt, B, P, table, keep = self._table(levels)
        dev = keep[0].device
        K, ai_ptr, cnt_ptr, cnt64, keep2 = self._rows(B, dev, anchor_index, count, A * P)
        knn = torch.empty(B, K, dtype=torch.float32, device=dev)
        idx = torch.empty(B, K, dtype=torch.int32, device=dev)
        cls = torch.empty(B, K, dtype=torch.int32, device=dev)
        bank, norms, bcls, _ = self._setup()
        ws = self._workspace(B * K, self.k, self.splits, dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(_lib.load().effdet_feature_knn_score(st, dt, *table, self.F, A, B, K, ai_ptr, cnt_ptr, cnt64, int(self.normalize), self.k,
                                                        self.splits, self.M, bank.data_ptr(), norms.data_ptr(), bcls.data_ptr(),
                                                        knn.data_ptr(), idx.data_ptr(), cls.data_ptr(), ws.data_ptr(), ws.numel()),
                   'effdet_feature_knn_score')
        return {'knn': knn, 'knn_index': idx, 'knn_class': cls}

    def score(self, levels, anchor_index, count=None):
        """Scores of the rows anchor_index [B, K] (int64): dict(knn [B, K] float32 = minus the SQUARED distance to the k-th nearest
        bank row, knn_index, knn_class [B, K] int32); rows at or beyond count[b] hold 0, -1, -1."""
        if anchor_index is None:
            raise ValueError('score() takes an anchor_index; score_cells() scores every cell')
        return self._score(levels, anchor_index, count, self.A)

    def score_cells(self, levels):
        """The same keys for every cell of the pyramid, [B, P]."""
        return self._score(levels, None, None, 1)

    # ---- state -----------------------------------------------------------------------------------------------------------
    def _geometry(self):
        return {'num_features': self.F, 'num_anchors': self.A, 'num_classes': self.C or None, 'normalize': self.normalize}

    def state_dict(self):
        bank, norms, bcls, _ = self._setup()
        size, seen, lost = self._counts()
        d = dict(self._geometry(), rows=bank[:size, :self.F].cpu(), norms=norms[:size].cpu(), classes=bcls[:size].cpu(), size=size, seen=seen,
                 lost=lost, sample_every=self.sample_every, k=self.k, fitted=self.M is not None)
        return d

    def _check_geometry(self, d, what):
        for key, mine in self._geometry().items():
            if d[key] != mine:
                raise ValueError('%s: %s differs (%r, %r)' % (what, key, d[key], mine))

    def _put(self, at, d):
        """rows of a state dict -> bank rows [at, at + n); n is cut at the capacity; returns (stored, dropped)"""
        bank, norms, bcls, _ = self._setup()
        n = int(d['size'])
        stored = max(min(n, self.capacity - at), 0)
        bank[at:at + stored, :self.F] = torch.as_tensor(d['rows'])[:stored].to(device=self.device, dtype=torch.float32)
        bank[at:at + stored, self.F:] = 0
        norms[at:at + stored] = torch.as_tensor(d['norms'])[:stored].to(device=self.device, dtype=torch.float32)
        bcls[at:at + stored] = torch.as_tensor(d['classes'])[:stored].to(device=self.device, dtype=torch.int32)
        return stored, n - stored

    def load_state_dict(self, d):
        self._check_geometry(d, 'load_state_dict')
        stored, dropped = self._put(0, d)
        self.counters.copy_(torch.tensor([stored, int(d['seen']), int(d['lost']) + dropped], dtype=torch.int64))
        self.k = int(d.get('k', self.k))
        self.M = None
        if d.get('fitted'):
            self.fit()
        return self

    def merge_(self, other):
        """Append the bank of another KNNFeatureOOD (or of its state dict) in its row order, e.g. another rank's; `seen` and
        `lost` add up; fit() again afterwards.  Reads the counters (synchronises)."""
        od = other.state_dict() if isinstance(other, KNNFeatureOOD) else other
        self._check_geometry(od, 'merge_')
        size, seen, lost = self._counts()
        stored, dropped = self._put(size, od)
        self.counters.copy_(torch.tensor([size + stored, seen + int(od['seen']), lost + int(od['lost']) + dropped], dtype=torch.int64))
        self.M = None
        return self
