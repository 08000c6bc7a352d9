"""Logit-space OOD scores on the device (csrc/logit_ood.hip): the scores every OOD benchmark reports next to the
energy, from one read of each row of class logits.

    lo = LogitOOD(config.num_classes)
    bench = DetBenchPredict(model, feature_ood=[lo])        # last_ood gains msp, neg_entropy, gen, joint_energy, predicted_class
    lo.add_detections(model(x)[0], bench.last_ood['anchor_index'], bench.last_count)     # in-distribution batches
    lo.fit()                                                # ... and kl_matching, kl_class, standardized_max_logit

Per row z of C logits (float32, or bfloat16 widened exactly), u = z / temperature, in float32:

    m = max u, k* = the lowest argmax, e_k = exp(u_k - m), s = sum e, lse = m + log s, l_k = u_k - lse, p_k = exp(l_k)
    predicted_class = k*;  msp = exp(m - lse);  neg_entropy = sum p_k l_k
    gen          = -sum over the top_m largest u_k of exp(gamma (l_k + q_k)),  q_k = log1p(-p_k), q_k* = log(sum_{k != k*} e_k) - log s
                   (generalized entropy, Liu et al. 2023, in the log domain: p^gamma never passes through an underflowed p and
                   1 - p never cancels)
    joint_energy = sum_k softplus(z_k)  (Wang et al. 2021: the energy of a multi-label, sigmoid-trained head; no temperature)

and, after `fit`, with the statistics n_c, P_c = sum p (temperature 1), a_c = sum max z, b_c = sum (max z)^2 per predicted class:

    kl_matching  = -min_c kl_c,  kl_c = neg_entropy - sum_k p_k log D_ck  (p, neg_entropy at temperature 1; Hendrycks et al. 2022),
                   D_c = (1 - smoothing) P_c / n_c + smoothing / C;  kl_class = argmin (ties to the lower class)
    standardized_max_logit = (max z - mu_k*) / sigma_k*  (Jung et al. 2021; classes with fewer than 2 rows use the pooled moments)

Every float key reads higher as more in-distribution, so `ood.OODEvaluator.add_detections` takes them unchanged.  `add*`
accumulate in float64 on the device (no host synchronisation, capturable in a graph, one fixed summation order, no atomics);
`fit` reads C * (C + 3) numbers back once.  There is no CPU fallback."""
import numpy as np
import torch

from . import _lib
from .ood_features import MAX_CLASSES, _PyramidRows


def finalize(n_c, P_c, a_c, b_c, smoothing=1e-6, std_floor=1e-3):
    """Statistics -> scoring parameters, float64 numpy (parameter-sized host glue, once per fit).
    Returns dict(log_d [C, C] (row c: log D_c; 0 for a class without rows), kl_inf [C] (0, +inf for a class without rows),
    mu, sigma, inv_sigma [C], have [C] bool, n)."""
    n_c = np.asarray(n_c, np.int64)
    P_c, a_c, b_c = np.asarray(P_c, np.float64), np.asarray(a_c, np.float64), np.asarray(b_c, np.float64)
    C = n_c.shape[0]
    if not 0.0 < float(smoothing) <= 1.0:
        raise ValueError('smoothing must lie in (0, 1], got %r' % (smoothing,))
    if not float(std_floor) > 0.0:
        raise ValueError('std_floor must be > 0, got %r' % (std_floor,))
    have = n_c > 0
    n = int(n_c.sum())
    if not have.any():
        raise ValueError('LogitOOD.fit: no rows were added')
    log_d = np.zeros((C, C))
    D = (1.0 - float(smoothing)) * P_c[have] / n_c[have, None] + float(smoothing) / C
    log_d[have] = np.log(D)
    mu_p = a_c.sum() / n
    sd_p = np.sqrt(max(b_c.sum() / n - mu_p * mu_p, 0.0))
    own = n_c >= 2
    nn = np.maximum(n_c, 1)
    mu = np.where(own, a_c / nn, mu_p)
    sigma = np.where(own, np.sqrt(np.maximum(b_c / nn - (a_c / nn) ** 2, 0.0)), sd_p)
    sigma = np.maximum(sigma, float(std_floor))
    return {'log_d': log_d, 'kl_inf': np.where(have, 0.0, np.inf), 'mu': mu, 'sigma': sigma, 'inv_sigma': 1.0 / sigma, 'have': have, 'n': n}


class LogitOOD(_PyramidRows):
    """Logit-space scores of rows of class logits (module docstring).  1 <= num_classes <= 1024; temperature > 0 applies to msp,
    neg_entropy, gen and predicted_class; top_m is clipped to num_classes.  Logits are a [B, N, C] tensor (float32 or bfloat16,
    any non-negative image and anchor strides, class stride 1) or the model's per-level [B, A * C, H, W] list."""
    KEYS = ('msp', 'neg_entropy', 'gen', 'joint_energy', 'predicted_class', 'kl_matching', 'kl_class', 'standardized_max_logit')
    FITTED_KEYS = ('kl_matching', 'kl_class', 'standardized_max_logit')
    WANTS_CLASS_LOGITS = True                 # DetBenchPredict passes the packed class logits instead of the pyramid

    def __init__(self, num_classes, temperature=1.0, gamma=0.1, top_m=10, device='cuda'):
        self.C = int(num_classes)
        self.temperature, self.gamma, self.top_m = float(temperature), float(gamma), int(top_m)
        if not 1 <= self.C <= MAX_CLASSES:
            raise ValueError('num_classes must lie in [1, %d], got %d' % (MAX_CLASSES, self.C))
        if not (self.temperature > 0.0 and np.isfinite(self.temperature)):
            raise ValueError('temperature must be > 0, got %r' % (temperature,))
        if not np.isfinite(self.gamma):
            raise ValueError('gamma must be finite, got %r' % (gamma,))
        if self.top_m < 1:
            raise ValueError('top_m must be >= 1, got %d' % self.top_m)
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('LogitOOD runs on the GPU (no CPU fallback)')
        self.smoothing = self.std_floor = None   # set by fit()
        self.params = None                       # float64 numpy results of the last fit (finalize())
        self._dev = None                         # their float32 uploads: log D [Cp, Cp], kl_inf [Cp], mu [C], inv_sigma [C]
        self._stats = None

    # ---- storage ---------------------------------------------------------------------------------------------------------
    def _setup(self):
        if self._stats is None:
            dev, C = self.device, self.C
            self._stats = (torch.zeros(C, dtype=torch.int64, device=dev), torch.zeros(C, C, dtype=torch.float64, device=dev),
                           torch.zeros(C, dtype=torch.float64, device=dev), torch.zeros(C, dtype=torch.float64, device=dev))
        return self._stats

    n_c = property(lambda self: self._setup()[0])
    P_c = property(lambda self: self._setup()[1])
    a_c = property(lambda self: self._setup()[2])
    b_c = property(lambda self: self._setup()[3])

    def _logits(self, logits):
        """logits -> a [B, N, C] view the kernels can address"""
        if not torch.is_tensor(logits):
            from .effdet.bench import _packed
            outs = list(logits)
            if not outs or any(not torch.is_tensor(t) or t.dim() != 4 or t.shape[1] % self.C for t in outs):
                raise ValueError('logits: a [B, N, %d] tensor or a list of [B, A * %d, H, W] tensors' % (self.C, self.C))
            if outs[0].device.type != 'cuda':
                raise RuntimeError('LogitOOD: logits must be GPU tensors (no CPU fallback)')
            logits = _packed(outs, len(outs), self.C)
        if logits.device.type != 'cuda':
            raise RuntimeError('LogitOOD: logits must be GPU tensors (no CPU fallback)')
        if logits.dim() != 3 or logits.shape[2] != self.C:
            raise ValueError('logits: a [B, N, %d] tensor or a list of [B, A * %d, H, W] tensors' % (self.C, self.C))
        if logits.dtype not in (torch.float32, torch.bfloat16):
            raise RuntimeError('logits must be float32 or bfloat16')
        logits = logits.detach()
        if (self.C > 1 and logits.stride(2) != 1) or min(logits.stride()) < 0:
            logits = logits.contiguous()
        B, N = logits.shape[0], logits.shape[1]
        if B < 1 or N < 1 or N > 1 << 31:
            raise ValueError('B >= 1 and 1 <= N <= 2^31')
        return logits

    def _head(self, logits):
        """the leading arguments both entry points share"""
        B, N = logits.shape[0], logits.shape[1]
        return (0 if logits.dtype == torch.float32 else 1, logits.data_ptr(), logits.stride(0) if B > 1 else 0,
                logits.stride(1) if N > 1 else 0, self.C, B, N)

    # ---- fit -------------------------------------------------------------------------------------------------------------
    def clear(self):
        """Forget every row and the fit (a device-side reset, no synchronisation)."""
        for t in self._setup():
            t.zero_()
        self.smoothing = self.std_floor = self.params = self._dev = None

    def add(self, logits, anchor_index=None, count=None, min_max_logit=None):
        """Add rows to the statistics of their predicted class.  Row (b, j) is anchor anchor_index[b, j] (int64 [B, K]; None: anchor
        j, the dense form with K = N); it counts when j < count[b] (None: all) and, with min_max_logit, when max z >= it."""
        logits = self._logits(logits)
        dev = logits.device
        B, N = logits.shape[0], logits.shape[1]
        K, ai_ptr, cnt_ptr, cnt64, keep = self._rows(B, dev, anchor_index, count, N)
        if min_max_logit is not None and not np.isfinite(float(min_max_logit)):
            raise ValueError('min_max_logit must be finite or None')
        lib = _lib.load()
        st, ws = self._stream_ws(dev, lib.effdet_logit_ood_workspace_bytes(B * K, self.C), B * K)
        n_c, P_c, a_c, b_c = self._setup()
        _lib.check(lib.effdet_logit_ood_fit(st, *self._head(logits), K, ai_ptr, cnt_ptr, cnt64, self.temperature,
                                            int(min_max_logit is not None), float(min_max_logit or 0.0), n_c.data_ptr(), P_c.data_ptr(),
                                            a_c.data_ptr(), b_c.data_ptr(), ws.data_ptr(), ws.numel()), 'effdet_logit_ood_fit')

    def add_detections(self, logits, anchor_index, count):
        """Add the kept detections of a `DetBenchPredict` pass: anchor_index = bench.last_ood['anchor_index'], count =
        bench.last_count."""
        if anchor_index is None:
            raise ValueError('add_detections() takes an anchor_index; add() takes every anchor')
        self.add(logits, anchor_index, count)

    def fit(self, smoothing=1e-6, std_floor=1e-3):
        """Statistics -> class templates and max-logit moments (`finalize`; reads C * (C + 3) numbers back, synchronises).
        ValueError when no class has rows."""
        n_c, P_c, a_c, b_c = self._setup()
        p = finalize(n_c.cpu().numpy(), P_c.cpu().numpy(), a_c.cpu().numpy(), b_c.cpu().numpy(), smoothing, std_floor)
        C, Cp = self.C, (self.C + 15) // 16 * 16
        log_d, kl_inf = np.zeros((Cp, Cp), np.float32), np.full(Cp, np.inf, np.float32)
        log_d[:C, :C], kl_inf[:C] = p['log_d'], p['kl_inf']
        self._dev = tuple(torch.from_numpy(a).to(self.device) for a in (log_d, kl_inf, p['mu'].astype(np.float32), p['inv_sigma'].astype(np.float32)))
        self.params, self.smoothing, self.std_floor = p, float(smoothing), float(std_floor)
        return self

    # ---- score -----------------------------------------------------------------------------------------------------------
    def _score(self, logits, anchor_index, count):
        logits = self._logits(logits)
        dev = logits.device
        B, N = logits.shape[0], logits.shape[1]
        K, ai_ptr, cnt_ptr, cnt64, keep = self._rows(B, dev, anchor_index, count, N)
        out = {k: torch.empty(B, K, dtype=torch.int64 if k.endswith('class') else torch.float32, device=dev)
               for k in self.KEYS if self._dev is not None or k not in self.FITTED_KEYS}
        fitted = [None] * 4 if self._dev is None else [t.data_ptr() for t in self._dev]
        ptr = lambda k: out[k].data_ptr() if k in out else None
        st, _ = self._stream_ws(dev)
        _lib.check(_lib.load().effdet_logit_ood_score(st, *self._head(logits), K, ai_ptr, cnt_ptr, cnt64, self.temperature, self.gamma,
                                                      self.top_m, *fitted, ptr('msp'), ptr('neg_entropy'), ptr('gen'), ptr('joint_energy'),
                                                      ptr('predicted_class'), ptr('kl_matching'), ptr('kl_class'),
                                                      ptr('standardized_max_logit')), 'effdet_logit_ood_score')
        return out

    def score(self, logits, anchor_index, count=None):
        """Scores of the rows anchor_index [B, K] (int64): a dict of [B, K] tensors, float32 and int64 for the two class keys; rows
        at or beyond count[b] hold 0 and -1 like the zero-padded detections.  The three fitted keys are present after fit()."""
        if anchor_index is None:
            raise ValueError('score() takes an anchor_index; score_anchors() scores every anchor')
        return self._score(logits, anchor_index, count)

    def score_anchors(self, logits):
        """The same keys for every anchor, [B, N]."""
        return self._score(logits, None, None)

    # ---- state -----------------------------------------------------------------------------------------------------------
    def state_dict(self):
        n_c, P_c, a_c, b_c = self._setup()
        d = {'num_classes': self.C, 'temperature': self.temperature, 'gamma': self.gamma, 'top_m': self.top_m, 'n_c': n_c.cpu(),
             'P_c': P_c.cpu(), 'a_c': a_c.cpu(), 'b_c': b_c.cpu()}
        if self.smoothing is not None:
            d['smoothing'], d['std_floor'] = self.smoothing, self.std_floor
        return d

    def load_state_dict(self, d):
        if d['num_classes'] != self.C:
            raise ValueError('state dict of another geometry')
        for dst, k in zip(self._setup(), ('n_c', 'P_c', 'a_c', 'b_c')):
            dst.copy_(torch.as_tensor(d[k]).to(dst.dtype))
        self.temperature, self.gamma, self.top_m = float(d.get('temperature', self.temperature)), float(d.get('gamma', self.gamma)), int(d.get('top_m', self.top_m))
        self.smoothing = self.std_floor = self.params = self._dev = None
        if d.get('smoothing') is not None:
            self.fit(d['smoothing'], d['std_floor'])
        return self

    def merge_(self, other):
        """Add the statistics of another LogitOOD (or of its state dict), e.g. another rank's; fit() again afterwards."""
        od = other.state_dict() if isinstance(other, LogitOOD) else other
        if od['num_classes'] != self.C:
            raise ValueError('merge_: another geometry')
        for dst, k in zip(self._setup(), ('n_c', 'P_c', 'a_c', 'b_c')):
            dst.add_(torch.as_tensor(od[k]).to(device=self.device, dtype=dst.dtype))
        self.smoothing = self.std_floor = self.params = self._dev = None
        return self
