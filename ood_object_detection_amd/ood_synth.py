"""Virtual outlier synthesis on the device (csrc/outlier_synth.hip): VOS's sampler (Du et al. 2022).  Class-conditional
Gaussians with a tied covariance are fitted to the penultimate features of the class head; per class S candidates are drawn and the
k least likely are kept - the outlier rows that `ood_train.EnergyRegularizer`'s 'logistic' form trains the energy on.

    synth = OutlierSynthesizer(config.fpn_channels, config.num_classes, num_anchors, candidates=10000, keep=1, min_count=64)
    synth.add(features, cls_targets)                     # any number of batches; FeatureOOD's statistics (n_c, s_c, S)
    synth.fit()                                          # the one host read: mu, L = cholesky(cov), valid = n_c >= min_count
    out = synth.sample()                                 # rows [C, k, F], index, r2, log_density [C, k], roles [C * k]
    loss, stats = virtual_outlier_loss(reg, class_out, roles, synth, weight, bias)           # ood_train

With x = mu_c + L eps the Mahalanobis distance of x is |eps|^2, so the least likely candidate is the one with the largest |eps|^2:
the selection works on the norms alone, L is applied to the k kept rows of a class only, and the S x F candidates are never stored.
The normals come from the counter-based generator Philox4x32-10: every number is a function of (seed, draw, class, candidate,
feature) alone, so two runs, a graph replay and any grouping of the classes into calls give the same bits, and draw t is followed
by draw t + 1 whether the call runs eagerly or as a replay.  `fit` copies into device buffers allocated once, so a captured
`sample` sees a new fit.  There is no CPU fallback."""
import numpy as np
import torch

from . import _lib
from .ood_features import WIDTHS, FeatureOOD, finalize

MAX_CLASSES = 1024
MAX_CANDIDATES = 1 << 20
MAX_ENTRIES = 1 << 26          # classes * candidates of one call
MAX_ROWS = 1 << 20             # classes * keep of one call
KEYS = ('rows', 'index', 'r2', 'log_density', 'roles')


def gaussian_factors(n_c, s_c, S, shrinkage=0.0, min_count=1):
    """Statistics -> what the sampler reads, float64 numpy: dict(mu [C, F], L [F, F] lower Cholesky factor of the tied covariance,
    log_const = -sum log L_dd - F / 2 log(2 pi), valid [C] bool = n_c >= min_count).  Raises like `ood_features.finalize`."""
    p = finalize(n_c, s_c, S, shrinkage)
    L = np.linalg.cholesky(p['cov'])
    F = L.shape[0]
    log_const = -float(np.log(L.diagonal()).sum()) - 0.5 * F * float(np.log(2.0 * np.pi))
    return {'mu': p['mu'], 'L': L, 'cov': p['cov'], 'log_const': log_const, 'valid': np.asarray(n_c, np.int64) >= int(min_count), 'n': p['n']}


class OutlierSynthesizer:
    """The sampler of virtual outliers (module docstring).  num_features: a BiFPN width (`ood_features.WIDTHS`);
    num_classes <= 1024; candidates (S) <= 2^20 with num_classes * S <= 2^26; 1 <= keep (k) <= S with num_classes * k <= 2^20.
    statistics: a `FeatureOOD` of the same geometry to share (one add* pass then fits both), or None: the object owns one.
    min_count: a class with fewer rows at the last fit is not valid - its rows are zeros and their role is -1 (default: 1)."""

    def __init__(self, num_features, num_classes, num_anchors, statistics=None, candidates=10000, keep=1, min_count=1, seed=0,
                 device='cuda'):
        self.F, self.C, self.A = int(num_features), int(num_classes), int(num_anchors)
        self.S, self.k, self.min_count, self.seed = int(candidates), int(keep), int(min_count), int(seed)
        if self.F not in WIDTHS:             # (the kernels take any multiple of 4 up to 512; the statistics take these)
            raise ValueError('num_features must be one of %r, got %d' % (WIDTHS, self.F))
        if not 1 <= self.C <= MAX_CLASSES:
            raise ValueError('num_classes must lie in [1, %d], got %d' % (MAX_CLASSES, self.C))
        if self.A < 1:
            raise ValueError('num_anchors must be >= 1')
        if not 1 <= self.S <= MAX_CANDIDATES or self.C * self.S > MAX_ENTRIES:
            raise ValueError('candidates must lie in [1, 2^20] with num_classes * candidates <= 2^26, got %d' % self.S)
        if not 1 <= self.k <= self.S or self.C * self.k > MAX_ROWS:
            raise ValueError('keep must lie in [1, candidates] with num_classes * keep <= 2^20, got %d' % self.k)
        if self.min_count < 1:
            raise ValueError('min_count must be >= 1')
        if not 0 <= self.seed < 1 << 64:
            raise ValueError('seed must lie in [0, 2^64)')
        if statistics is not None:
            if not isinstance(statistics, FeatureOOD):
                raise ValueError('statistics must be a FeatureOOD')
            if (statistics.F, statistics.C, statistics.A) != (self.F, self.C, self.A):
                raise ValueError('statistics of another geometry')
            device = statistics.device
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('OutlierSynthesizer runs on the GPU (no CPU fallback)')
        self.statistics = statistics if statistics is not None else FeatureOOD(self.F, self.C, self.A, device=self.device)
        self.params = None                   # float64 numpy results of the last fit (gaussian_factors())
        self.shrinkage = None
        self._buf = None
        self._ws = {}

    fitted = property(lambda self: self.params is not None)

    # ---- statistics --------------------------------------------------------------------------------------------------------------
    def add(self, *args, **kwargs):
        """`FeatureOOD.add` of the statistics: rows of the feature space with their classes (no synchronisation, capturable)."""
        self.statistics.add(*args, **kwargs)

    def add_targets(self, levels, cls_targets):
        self.statistics.add_targets(levels, cls_targets)

    def clear(self):
        """Forget every row and the fit (device-side resets; the draw counter and the seed stay)."""
        self.statistics.clear()
        self.params = self.shrinkage = None
        if self._buf is not None:
            self._buf['valid'].zero_()

    # ---- fit ---------------------------------------------------------------------------------------------------------------------
    def _buffers(self):
        if self._buf is None:
            dev, F, C = self.device, self.F, self.C
            self._buf = {'mu': torch.zeros(C, F, dtype=torch.float32, device=dev), 'U': torch.zeros(F, F, dtype=torch.float32, device=dev),
                         'log_const': torch.zeros(1, dtype=torch.float32, device=dev), 'valid': torch.zeros(C, dtype=torch.int8, device=dev),
                         'draw': torch.zeros(1, dtype=torch.int64, device=dev)}
        return self._buf

    def _upload(self, p):
        b = self._buffers()
        b['mu'].copy_(torch.from_numpy(p['mu'].astype(np.float32)))
        b['U'].copy_(torch.from_numpy(np.ascontiguousarray(p['L'].T).astype(np.float32)))
        b['log_const'].copy_(torch.tensor([p['log_const']], dtype=torch.float32))
        b['valid'].copy_(torch.from_numpy(p['valid'].astype(np.int8)))

    def fit(self, shrinkage=0.0):
        """Statistics -> mu, L = cholesky(cov), log_const and valid in float64 numpy (`gaussian_factors`; reads (C + F) * F + C
        numbers back, synchronises), copied in place into the device buffers `sample` reads.  Raises like `FeatureOOD.fit`."""
        st = self.statistics
        p = gaussian_factors(st.n_c.cpu().numpy(), st.s_c.cpu().numpy(), st.S.cpu().numpy(), shrinkage, self.min_count)
        self._upload(p)
        self.params, self.shrinkage = p, float(shrinkage)
        return self

    def set_gaussians(self, mu, L, valid=None):
        """Fit by hand: mu [C, F], L [F, F] lower triangular with a positive diagonal (float64 array-likes), valid [C] bool or None
        (all).  The same in-place upload as `fit`."""
        mu, L = np.asarray(mu, np.float64), np.asarray(L, np.float64)
        if mu.shape != (self.C, self.F) or L.shape != (self.F, self.F):
            raise ValueError('mu must be [%d, %d] and L [%d, %d]' % (self.C, self.F, self.F, self.F))
        if np.triu(L, 1).any() or not (L.diagonal() > 0).all() or not (np.isfinite(mu).all() and np.isfinite(L).all()):
            raise ValueError('L must be lower triangular with a positive diagonal, mu and L finite')
        valid = np.ones(self.C, bool) if valid is None else np.asarray(valid, bool)
        if valid.shape != (self.C,):
            raise ValueError('valid must be [%d]' % self.C)
        log_const = -float(np.log(L.diagonal()).sum()) - 0.5 * self.F * float(np.log(2.0 * np.pi))
        p = {'mu': mu, 'L': L, 'cov': L @ L.T, 'log_const': log_const, 'valid': valid, 'n': None}
        self._upload(p)
        self.params, self.shrinkage = p, None
        return self

    # ---- sample ------------------------------------------------------------------------------------------------------------------
    def _classes(self, classes):
        if classes is None:
            return self.C, None
        if not torch.is_tensor(classes):
            classes = torch.as_tensor(list(classes), dtype=torch.int32)
            if classes.numel() and (int(classes.min()) < 0 or int(classes.max()) >= self.C):
                raise ValueError('classes must lie in [0, %d)' % self.C)
            classes = classes.to(self.device)
        if classes.device.type != 'cuda':
            raise RuntimeError('OutlierSynthesizer: classes must be a GPU tensor (no CPU fallback)')
        if classes.dtype != torch.int32 or classes.dim() != 1 or not 1 <= classes.numel() <= MAX_CLASSES or classes.device != self.device:
            raise ValueError('classes: between 1 and %d int32 class ids on the device of the sampler' % MAX_CLASSES)
        return classes.numel(), classes.contiguous()

    def sample(self, classes=None, advance=True):
        """One draw: dict(rows [n, k, F] float32, index [n, k] int32, r2, log_density [n, k] float32, roles [n * k] int8) for the
        classes `classes` (None: all C; a sequence of ids; or an int32 device tensor, which a graph may capture; an id outside
        [0, C) in a tensor gives an invalid class).  The draw counter advances by one on the device unless advance is False - the
        way to sample one draw in several calls.  No synchronisation; the outputs are new tensors."""
        if self.params is None:
            raise RuntimeError('OutlierSynthesizer: fit() comes before sample()')
        n, ids = self._classes(classes)
        lib, b, dev = _lib.load(), self._buffers(), self.device
        if n * self.S > MAX_ENTRIES or n * self.k > MAX_ROWS:
            raise ValueError('too many classes for one call')
        out = {'rows': torch.empty(n, self.k, self.F, dtype=torch.float32, device=dev),
               'index': torch.empty(n, self.k, dtype=torch.int32, device=dev),
               'r2': torch.empty(n, self.k, dtype=torch.float32, device=dev),
               'log_density': torch.empty(n, self.k, dtype=torch.float32, device=dev),
               'roles': torch.empty(n * self.k, dtype=torch.int8, device=dev)}
        need = lib.effdet_outlier_synth_workspace_bytes(n, self.S)
        if need <= 0:
            raise ValueError('no workspace for %d classes of %d candidates' % (n, self.S))
        ws = self._ws.get(n)                 # owned by the object: a captured call keeps reading the same memory
        if ws is None:
            ws = self._ws[n] = torch.empty(need, dtype=torch.uint8, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(lib.effdet_outlier_synth(st, self.F, self.C, n, None if ids is None else ids.data_ptr(), self.S, self.k, self.seed,
                                            b['draw'].data_ptr(), int(bool(advance)), b['mu'].data_ptr(), b['U'].data_ptr(),
                                            b['log_const'].data_ptr(), b['valid'].data_ptr(), out['rows'].data_ptr(),
                                            out['index'].data_ptr(), out['r2'].data_ptr(), out['log_density'].data_ptr(),
                                            out['roles'].data_ptr(), ws.data_ptr(), ws.numel()), 'effdet_outlier_synth')
        return out

    # ---- state -------------------------------------------------------------------------------------------------------------------
    @property
    def draw(self):
        """The number of the next draw (reads one int64 back, synchronises)."""
        return int(self._buffers()['draw'].item())

    def seek(self, draw):
        """Make `draw` (0 <= draw < 2^63) the number of the next draw: a device-side fill, seen by the next replay of a captured call."""
        if not 0 <= int(draw) < 1 << 63:
            raise ValueError('draw must lie in [0, 2^63)')
        self._buffers()['draw'].fill_(int(draw))
        return self

    def state_dict(self):
        d = {'num_features': self.F, 'num_classes': self.C, 'num_anchors': self.A, 'candidates': self.S, 'keep': self.k,
             'min_count': self.min_count, 'seed': self.seed, 'draw': self.draw, 'statistics': self.statistics.state_dict()}
        if self.params is not None and self.shrinkage is not None:
            d['shrinkage'] = self.shrinkage
        return d

    def load_state_dict(self, d):
        if (d['num_features'], d['num_classes'], d['num_anchors']) != (self.F, self.C, self.A):
            raise ValueError('state dict of another geometry')
        if (d['candidates'], d['keep']) != (self.S, self.k):
            raise ValueError('state dict of another candidates / keep (%d, %d)' % (d['candidates'], d['keep']))
        stats = dict(d['statistics'])
        stats.pop('shrinkage', None)         # (the shared FeatureOOD keeps its own fit; the sampler's is redone below)
        self.statistics.load_state_dict(stats)
        self.min_count, self.seed = int(d['min_count']), int(d['seed'])
        self.seek(d['draw'])
        self.params = self.shrinkage = None
        if d.get('shrinkage') is not None:
            self.fit(d['shrinkage'])
        return self
