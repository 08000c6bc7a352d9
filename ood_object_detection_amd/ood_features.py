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
    bench = DetBenchPredict(model, feature_ood=[maha, f])   # last_ood gains knn, knn_index, knn_class as well

`SubspaceFeatureOOD` (csrc/feature_subspace.hip) scores a row by its component outside the principal subspace of the
in-distribution features: the norm of that component (`residual`), its Mahalanobis distance within the low-variance directions
(`partial_mahalanobis`, Kamoi & Kobayashi 2020) and ViM (Wang et al. 2022), which takes the residual, scaled by alpha, off a logit
score.  It needs no statistics beyond those `FeatureOOD.add*` accumulates, so it can share them, and its fit cannot fail:

    sub = SubspaceFeatureOOD(config.fpn_channels, config.num_classes, num_anchors, statistics=maha)   # one add* pass fits both
    sub.fit(explained=0.9)
    sub.calibrate(levels, anchor_index, count, bench.last_ood['energy']); sub.finish_calibration()     # alpha, for vim
    bench = DetBenchPredict(model, feature_ood=[maha, f, sub])   # last_ood gains residual, partial_mahalanobis, vim as well"""
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


def finalize_subspace(n_c, s_c, S, dim=None, explained=None, floor=1e-6):
    """Statistics -> the residual subspace, float64 numpy (parameter-sized host glue, once per fit).
    mu0 = sum_c s_c / n, cov0 = S / n - mu0 mu0^T (symmetrised) = U diag(lambda) U^T with lambda descending.  The principal
    dimension D is `dim` (0 <= dim <= F - 1), or the smallest D whose leading eigenvalues sum to at least explained * trace
    (0 < explained <= 1; capped at F - 1), or F // 2.  Returns dict(mu0 [F], R = U[:, D:] [F, F - D], lambda [F],
    inv_lambda [F - D] = 1 / max(lambda_i, floor * trace / F) of the residual directions, dim, n)."""
    n_c = np.asarray(n_c, np.int64)
    s_c, S = np.asarray(s_c, np.float64), np.asarray(S, np.float64)
    F = s_c.shape[1]
    n = int(n_c.sum())
    if n < 1:
        raise ValueError('SubspaceFeatureOOD.fit: no rows were added')
    if dim is not None and explained is not None:
        raise ValueError('pass dim or explained, not both')
    if not (float(floor) >= 0.0):
        raise ValueError('floor must be >= 0')
    mu0 = s_c.sum(0) / n
    cov0 = S / n - np.outer(mu0, mu0)
    lam, U = np.linalg.eigh(0.5 * (cov0 + cov0.T))
    lam, U = lam[::-1].copy(), U[:, ::-1].copy()
    trace = float(lam.sum())
    if dim is not None:
        D = int(dim)
        if D != dim or not 0 <= D <= F - 1:
            raise ValueError('dim must be an integer in [0, %d], got %r' % (F - 1, dim))
    elif explained is not None:
        if not 0.0 < float(explained) <= 1.0:
            raise ValueError('explained must lie in (0, 1], got %r' % (explained,))
        D = min(int(np.searchsorted(np.cumsum(lam), float(explained) * trace, side='left')) + 1, F - 1)
    else:
        D = F // 2
    low = float(floor) * trace / F
    with np.errstate(divide='ignore'):
        inv = 1.0 / np.maximum(lam[D:], low)
    return {'mu0': mu0, 'R': U[:, D:].copy(), 'lambda': lam, 'inv_lambda': inv, 'dim': D, 'n': n}


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

    def _classes(self, classes, B, K, dev):
        """classes [B, K] -> (pointer, dtype code, image stride, entry stride, tensor to keep alive)"""
        if not torch.is_tensor(classes) or classes.device != dev or classes.dim() != 2 or classes.shape[0] != B:
            raise ValueError('classes: a [B, K] tensor on the device of the features')
        if classes.dtype not in (torch.int32, torch.int64, torch.float32):
            raise ValueError('classes must be int32, int64 or float32')
        if classes.shape[1] != K:
            raise ValueError('classes must be [B, %d] like the rows' % K)
        classes = classes.detach()
        if min(classes.stride()) < 0:
            classes = classes.contiguous()
        return classes.data_ptr(), {torch.int32: 0, torch.int64: 1, torch.float32: 2}[classes.dtype], classes.stride(0), classes.stride(1), classes

    @staticmethod
    def _det_classes(det):
        """det [B, max_det, 6] of a `DetBenchPredict` pass -> its class column (class + 1)"""
        if not torch.is_tensor(det) or det.dim() != 3 or det.shape[2] != 6 or det.dtype != torch.float32:
            raise ValueError('det must be a float32 [B, max_det, 6] tensor')
        return det[..., 5]

    @staticmethod
    def _stream_ws(dev, need=None, rows=0):
        """(the current stream of dev, a workspace of `need` bytes of this call's own or None): the caching allocator hands it out
        per stream, so the sub-batch streams of a `DetBenchPredict` do not share one; inside a graph capture it comes from the
        graph's pool"""
        if need is not None and need <= 0:
            raise ValueError('between 1 and 2^27 rows per call, got %d' % rows)
        ws = None if need is None else torch.empty(need, dtype=torch.uint8, device=dev)
        return torch.cuda.current_stream(dev).cuda_stream, ws


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
        K, ai_ptr, cnt_ptr, cnt64, keep2 = self._rows(B, dev, anchor_index, count, self.A * P)
        cls_ptr, cdt, pitch, stride, classes = self._classes(classes, B, K, dev)
        n_c, s_c, S = self._setup()
        ws = self._workspace(B * K)
        st, _ = self._stream_ws(dev)
        _lib.check(_lib.load().effdet_feature_ood_fit(st, dt, *table, self.F, self.C, self.A, B, K, ai_ptr, cls_ptr, cdt, pitch, stride,
                                                      int(class_offset), cnt_ptr, cnt64, n_c.data_ptr(), s_c.data_ptr(), S.data_ptr(),
                                                      ws.data_ptr(), ws.numel()), 'effdet_feature_ood_fit')

    def add_detections(self, levels, det, anchor_index, count):
        """Add the kept detections of a `DetBenchPredict` pass: det [B, max_det, 6] (class + 1 in det[..., 5]),
        anchor_index = bench.last_ood['anchor_index'], count = bench.last_count."""
        self.add(levels, self._det_classes(det), anchor_index, count, class_offset=1)

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
        st, _ = self._stream_ws(dev)
        _lib.check(_lib.load().effdet_feature_ood_score(st, dt, *table, self.F, self.C, A, B, K, ai_ptr, cnt_ptr, cnt64,
                                                        *[t.data_ptr() for t in self._dev], maha.data_ptr(), rel.data_ptr(),
                                                        near.data_ptr()), 'effdet_feature_ood_score')
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
        """(stream, workspace) of a call: k = 0 for an append"""
        return self._stream_ws(dev, _lib.load().effdet_feature_knn_workspace_bytes(rows, self.F, k, splits), rows)

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
            cls_ptr, cdt, pitch, stride, classes = self._classes(classes, B, K, dev)
        bank, norms, bcls, counters = self._setup()
        st, ws = self._workspace(B * K, 0, 0, dev)
        _lib.check(_lib.load().effdet_feature_knn_append(st, dt, *table, self.F, self.C, self.A, B, K, ai_ptr, cls_ptr, cdt, pitch, stride,
                                                         int(class_offset), cnt_ptr, cnt64, int(self.normalize), self.sample_every,
                                                         self.capacity, bank.data_ptr(), norms.data_ptr(), bcls.data_ptr(),
                                                         counters.data_ptr(), ws.data_ptr(), ws.numel()), 'effdet_feature_knn_append')
        self.M = None

    def add_detections(self, levels, det, anchor_index, count):
        """Append the kept detections of a `DetBenchPredict` pass: det [B, max_det, 6] (class + 1 in det[..., 5]),
        anchor_index = bench.last_ood['anchor_index'], count = bench.last_count."""
        labels = self._det_classes(det)
        self.add(levels, labels if self.C else None, anchor_index, count, class_offset=1)

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
        st, ws = self._workspace(B * K, self.k, self.splits, dev)
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


class SubspaceFeatureOOD(_PyramidRows):
    """Subspace scores of pyramid rows (csrc/feature_subspace.hip).  With mu0 and R [F, F - D] of
    `finalize_subspace` (the eigenvectors of the pooled covariance beyond the D leading ones), per row in float32

        y = R^T (f - mu0),   r = |y|,   residual = -r,   partial_mahalanobis = -sum_i inv_lambda_i y_i^2,   vim = t - alpha r

    where t is a logit score of the row: -energy (the log-sum-exp) for logit='energy', max_logit for logit='max_logit'; `vim` is
    minus the score of Wang et al. 2022, so that a higher value means more in-distribution like every other key.  The origin is
    mu0 (the separable-conv class head has no `-(W^T)^+ b`).

    statistics: a `FeatureOOD` of the same geometry whose n_c / s_c / S are shared - one `add*` pass then fits both scorers - or
    None for statistics of this object's own; `add*` and `clear` go to it.  `fit` reads the statistics back (the one
    synchronisation) and cannot fail for want of rows.  alpha is given to `fit`, or measured: `calibrate` adds n, sum t and sum r
    over the valid rows of a call on the device (float64, one fixed order, no atomics, capturable in a graph) and
    `finish_calibration` sets alpha = sum t / sum r, ViM's rule.  That rule needs a positive mean logit score: the sigmoid heads of
    a detector can have a negative mean log-sum-exp over weak detections, and then `finish_calibration` refuses - calibrate on rows
    above a detection-score threshold (through `count`), or pass alpha to `fit`.  This is a property of the method.
    There is no CPU fallback."""
    KEYS = ('residual', 'partial_mahalanobis', 'vim')
    WANTS_LOGIT_SCORE = True                  # DetBenchPredict passes logit_score= (the gathered `logit` key) to score()
    LOGITS = ('energy', 'max_logit')

    def __init__(self, num_features, num_classes, num_anchors, statistics=None, logit='energy', device='cuda'):
        if logit not in self.LOGITS:
            raise ValueError('logit must be one of %r, got %r' % (self.LOGITS, logit))
        if statistics is None:
            statistics = FeatureOOD(num_features, num_classes, num_anchors, device=device)
        elif not isinstance(statistics, FeatureOOD):
            raise ValueError('statistics must be a FeatureOOD or None')
        elif (statistics.F, statistics.C, statistics.A) != (int(num_features), int(num_classes), int(num_anchors)):
            raise ValueError('statistics of another geometry')
        self.statistics = statistics
        self.F, self.C, self.A = statistics.F, statistics.C, statistics.A
        self.device = statistics.device
        self.logit = logit
        self.dim = self.floor = self.alpha = None     # set by fit() (alpha also by finish_calibration())
        self.params = None                            # float64 numpy results of the last fit (finalize_subspace())
        self._dev = None                              # (Rt [Rp][Fp], inv_lambda [Rp], mu0 [Fp]) float32 uploads
        self._cal = None

    # ---- statistics ------------------------------------------------------------------------------------------------------
    def add(self, *args, **kwargs):
        """`FeatureOOD.add` of the statistics object."""
        self.statistics.add(*args, **kwargs)

    def add_detections(self, levels, det, anchor_index, count):
        self.statistics.add_detections(levels, det, anchor_index, count)

    def add_targets(self, levels, cls_targets):
        self.statistics.add_targets(levels, cls_targets)

    def clear(self):
        """Forget every row (of the statistics object: a shared one is cleared for both scorers), the fit and the calibration."""
        self.statistics.clear()
        self.dim = self.floor = self.alpha = self.params = self._dev = None
        self.reset_calibration()

    # ---- fit -------------------------------------------------------------------------------------------------------------
    def fit(self, dim=None, explained=None, floor=1e-6, alpha=None):
        """Statistics -> residual directions (`finalize_subspace`; reads (C + F) * F + C numbers back, synchronises).  alpha: ViM's
        scale when it is known; otherwise it stays unset until `finish_calibration`."""
        st = self.statistics
        p = finalize_subspace(st.n_c.cpu().numpy(), st.s_c.cpu().numpy(), st.S.cpu().numpy(), dim, explained, floor)
        self._upload(p)
        self.params, self.dim, self.floor = p, p['dim'], float(floor)
        self.alpha = None if alpha is None else float(alpha)
        return self

    def _upload(self, p):
        F, Rn = self.F, self.F - p['dim']
        Fp, Rp = (F + 15) // 16 * 16, (Rn + 15) // 16 * 16
        Rt, il, mu0 = np.zeros((Rp, Fp), np.float32), np.zeros(Rp, np.float32), np.zeros(Fp, np.float32)
        Rt[:Rn, :F], il[:Rn], mu0[:F] = p['R'].T, p['inv_lambda'], p['mu0']
        self._dev = tuple(torch.from_numpy(a).to(self.device) for a in (Rt, il, mu0))

    # ---- calibration -----------------------------------------------------------------------------------------------------
    def _counters(self):
        if self._cal is None:
            self._cal = (torch.zeros(1, dtype=torch.int64, device=self.device), torch.zeros(2, dtype=torch.float64, device=self.device))
        return self._cal

    def reset_calibration(self):
        """Zero the three calibration counters (a device-side reset, no synchronisation)."""
        for t in self._counters():
            t.zero_()

    def _logit(self, logit_score, B, K, dev):
        if not torch.is_tensor(logit_score) or logit_score.device != dev or logit_score.dtype != torch.float32 or tuple(logit_score.shape) != (B, K):
            raise ValueError('logit_score: a float32 [B, %d] tensor on the device of the features' % K)
        logit_score = logit_score.detach()
        if min(logit_score.stride()) < 0:
            logit_score = logit_score.contiguous()
        return logit_score

    def calibrate(self, levels, anchor_index, count, logit_score):
        """Add the valid rows (j < count[b]) of a call to n, sum t, sum r on the device; t from logit_score (float32 [B, K], the
        `logit` key of `last_ood`; strided views are fine) by the sign rule, r under the current fit."""
        if self._dev is None:
            raise RuntimeError('SubspaceFeatureOOD: fit() comes before calibrate()')
        if anchor_index is None:
            raise ValueError('calibrate() takes an anchor_index')
        dt, B, P, table, keep = self._table(levels)
        dev = keep[0].device
        K, ai_ptr, cnt_ptr, cnt64, keep2 = self._rows(B, dev, anchor_index, count, self.A * P)
        ls = self._logit(logit_score, B, K, dev)
        Rt, il, mu0 = self._dev
        n, sums = self._counters()
        lib = _lib.load()
        st, ws = self._stream_ws(dev, lib.effdet_feature_subspace_workspace_bytes(B * K), B * K)
        _lib.check(lib.effdet_feature_subspace_calibrate(st, dt, *table, self.F, self.A, B, K, ai_ptr, cnt_ptr, cnt64, Rt.data_ptr(),
                                                         mu0.data_ptr(), Rt.shape[0], ls.data_ptr(), ls.stride(0), ls.stride(1),
                                                         int(self.logit == 'energy'), n.data_ptr(), sums.data_ptr(), ws.data_ptr(),
                                                         ws.numel()), 'effdet_feature_subspace_calibrate')

    def calibration(self):
        """(n, sum t, sum r) so far (synchronises)."""
        n, sums = self._counters()
        s = sums.cpu()
        return int(n.cpu()[0]), float(s[0]), float(s[1])

    def finish_calibration(self):
        """alpha = sum t / sum r over the calibrated rows (ViM's rule; reads three numbers, synchronises).  ValueError when no row
        was calibrated or the ratio is not positive - the mean logit score of weak detections of a sigmoid head can be negative:
        calibrate on rows above a detection-score threshold, or pass alpha to fit()."""
        n, st, sr = self.calibration()
        remedy = 'calibrate on rows above a detection-score threshold, or pass fit(alpha=...)'
        if n == 0:
            raise ValueError('SubspaceFeatureOOD.finish_calibration: no rows were calibrated: ' + remedy)
        alpha = st / sr if sr > 0.0 else float('nan')
        if not alpha > 0.0 or not np.isfinite(alpha):
            raise ValueError('SubspaceFeatureOOD.finish_calibration: sum t = %g over sum r = %g of %d rows gives no positive alpha: %s'
                             % (st, sr, n, remedy))
        self.alpha = alpha
        return self

    # ---- score -----------------------------------------------------------------------------------------------------------
    def _score(self, levels, anchor_index, count, A, logit_score):
        if self._dev is None:
            raise RuntimeError('SubspaceFeatureOOD: fit() comes before score()')
        dt, B, P, table, keep = self._table(levels)
        dev = keep[0].device
        K, ai_ptr, cnt_ptr, cnt64, keep2 = self._rows(B, dev, anchor_index, count, A * P)
        res = torch.empty(B, K, dtype=torch.float32, device=dev)
        pm = torch.empty_like(res)
        out = {'residual': res, 'partial_mahalanobis': pm}
        ls_ptr, pitch, stride, vim_ptr, alpha = None, 0, 0, None, 0.0
        if self.alpha is not None and logit_score is not None:
            ls = self._logit(logit_score, B, K, dev)
            out['vim'] = torch.empty_like(res)
            ls_ptr, pitch, stride, vim_ptr, alpha = ls.data_ptr(), ls.stride(0), ls.stride(1), out['vim'].data_ptr(), self.alpha
        Rt, il, mu0 = self._dev
        st, _ = self._stream_ws(dev)
        _lib.check(_lib.load().effdet_feature_subspace_score(st, dt, *table, self.F, A, B, K, ai_ptr, cnt_ptr, cnt64, Rt.data_ptr(),
                                                             il.data_ptr(), mu0.data_ptr(), Rt.shape[0], ls_ptr, pitch, stride,
                                                             int(self.logit == 'energy'), alpha, res.data_ptr(), pm.data_ptr(), vim_ptr),
                   'effdet_feature_subspace_score')
        return out

    def score(self, levels, anchor_index, count=None, logit_score=None):
        """Scores of the rows anchor_index [B, K] (int64): dict(residual, partial_mahalanobis [B, K] float32) and, once alpha is set
        and logit_score (float32 [B, K], the `logit` key of `last_ood`) is given, vim; rows at or beyond count[b] hold 0."""
        if anchor_index is None:
            raise ValueError('score() takes an anchor_index; score_cells() scores every cell')
        return self._score(levels, anchor_index, count, self.A, logit_score)

    def score_cells(self, levels):
        """residual and partial_mahalanobis for every cell of the pyramid, [B, P] (a cell has no logit score)."""
        return self._score(levels, None, None, 1, None)

    # ---- state -----------------------------------------------------------------------------------------------------------
    def state_dict(self):
        d = {k: v for k, v in self.statistics.state_dict().items() if k != 'shrinkage'}
        n, st, sr = self.calibration()
        d.update(dim=self.dim, floor=self.floor, alpha=self.alpha, logit=self.logit, calibration=(n, st, sr))
        return d

    def load_state_dict(self, d):
        """The statistics go to the statistics object (a shared `FeatureOOD` receives them too and loses its fit)."""
        self.statistics.load_state_dict({k: d[k] for k in ('num_features', 'num_classes', 'num_anchors', 'n_c', 's_c', 'S')})
        self.logit = d.get('logit', self.logit)
        if self.logit not in self.LOGITS:
            raise ValueError('logit must be one of %r, got %r' % (self.LOGITS, self.logit))
        self.dim = self.floor = self.alpha = self.params = self._dev = None
        n, sums = self._counters()
        cal = d.get('calibration', (0, 0.0, 0.0))
        n.copy_(torch.tensor([int(cal[0])], dtype=torch.int64))
        sums.copy_(torch.tensor([float(cal[1]), float(cal[2])], dtype=torch.float64))
        if d.get('dim') is not None:
            self.fit(dim=d['dim'], floor=d['floor'], alpha=d.get('alpha'))
        return self

    def merge_(self, other):
        """Add the statistics and the calibration counters of another SubspaceFeatureOOD (or of its state dict), e.g. another
        rank's; fit() again afterwards."""
        od = other.state_dict() if isinstance(other, SubspaceFeatureOOD) else other
        self.statistics.merge_({k: od[k] for k in ('num_features', 'num_classes', 'num_anchors', 'n_c', 's_c', 'S')})
        n, sums = self._counters()
        cal = od.get('calibration', (0, 0.0, 0.0))
        n.add_(torch.tensor([int(cal[0])], dtype=torch.int64, device=self.device))
        sums.add_(torch.tensor([float(cal[1]), float(cal[2])], dtype=torch.float64, device=self.device))
        self.dim = self.floor = self.alpha = self.params = self._dev = None
        return self
