"""Post-hoc calibration of the detection score on the device (csrc/calibration_eval.hip):

    p' = sigmoid(a logit(p~) + b),   p~ = p clamped to [2^-24, 1 - 2^-24]

`method='platt'` fits a and b, `method='temperature'` fits a alone (b = 0, T = 1 / a).  `target='tp'` fits the probability of a
true positive at the chosen IoU threshold; `target='iou'` the localisation-aware target of LaECE, y = IoU for a true positive
and 0 otherwise, as soft labels in the same cross-entropy.  With a > 0 the map is monotone, so calibrated rows keep the
non-increasing score order the evaluators need.

`fit` runs a damped Newton iteration on the unsorted entries a `CalibrationEvaluator` has accumulated: every iteration is two
launches (per-workgroup float64 partial sums of NLL, gradient and Hessian in a fixed order; one workgroup that adds them in
ascending order and advances a 16-double state block).  `max_iter` pairs are always enqueued - a converged state makes the rest
no-ops - so nothing is read back and `fit` -> `apply` -> evaluator chains and captures.  `finish()` is the one small copy.
The first `fit`, `apply` or `state` of a calibrator allocates its device blocks and uploads the starting state (a host-to-device
copy), and `load_state_dict` uploads (a, b): do either once eagerly before capturing a graph that uses the calibrator.

Not built: histogram binning and isotonic regression (not monotone in float32: they would break the score order), per-class
(a_c, b_c), the box-position / box-size dimensions of D-ECE, second-order autograd.  No CPU fallback.
"""
import torch

from . import _lib

METHODS = ('platt', 'temperature')
TARGETS = ('tp', 'iou')
STATE_DOUBLES = 16
_FIELDS = ('a', 'b', 'nll', 'trial_a', 'trial_b', 'step', 'dir_a', 'dir_b', 'nll_before', 'iterations', 'halvings', 'converged',
           'frozen', 'accepted', 'entries')


def _start_state(a=1.0, b=0.0):
    s = [0.0] * STATE_DOUBLES
    s[0], s[1], s[3], s[4], s[5] = a, b, a, b, 1.0
    return s


class DetectionCalibrator(object):

    def __init__(self, method='platt', target='tp', device='cuda:0'):
        if method not in METHODS:
            raise ValueError('method: one of %r, got %r' % (METHODS, method))
        if target not in TARGETS:
            raise ValueError('target: one of %r, got %r' % (TARGETS, target))
        self.method, self.target = method, target
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('the calibrator runs on the GPU (no CPU fallback)')
        self._state = None              # [16] float64 on the device, allocated on first use
        self._start = None
        self._partials = None
        self._host = None               # (a, b) known on the host: after finish() or load_state_dict()
        self._summary = None
        self._fitted = False            # a fit has been enqueued whose (a, b) the host has not read

    # ---- device blocks ----------------------------------------------------------------------------------------------------------------
    def _blocks(self):
        if self._state is None:
            self.lib = _lib.load()
            a, b = self._host if self._host is not None else (1.0, 0.0)
            self._state = torch.tensor(_start_state(a, b), dtype=torch.float64, device=self.device)
            self._start = torch.tensor(_start_state(), dtype=torch.float64, device=self.device)
        return self._state

    def _st(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    @property
    def state(self):
        """the [16] float64 state block on the device; (a, b) are its first two entries"""
        return self._blocks()

    # ---- fit --------------------------------------------------------------------------------------------------------------------------
    def fit(self, evaluator, threshold_index=0, max_iter=32):
        """Enqueue `max_iter` Newton iterations over `evaluator`'s accumulated entries (a CalibrationEvaluator on this device, or
        the `effdet.evaluator.CalibrationEvaluator` wrapper that `create_evaluator('calibration', ...)` returns) at
        IoU threshold `threshold_index`; no host read.  -> self"""
        evaluator = getattr(evaluator, 'device_evaluator', evaluator)      # the effdet.evaluator wrapper of create_evaluator
        if not hasattr(evaluator, 'entries'):
            raise TypeError('fit() takes a CalibrationEvaluator')
        if evaluator.device != self.device:
            raise RuntimeError('the evaluator lives on %s, the calibrator on %s' % (evaluator.device, self.device))
        T = len(evaluator.thresholds)
        if not 0 <= int(threshold_index) < T:
            raise ValueError('threshold_index must lie in [0, %d), got %r' % (T, threshold_index))
        if int(max_iter) < 1:
            raise ValueError('max_iter must be at least 1')
        state = self._blocks()
        scores, _, flags, iou, cursor = evaluator.entries()
        capacity = scores.numel()
        nb = self.lib.effdet_calibration_fit_workspace_bytes(capacity)
        if self._partials is None or self._partials.numel() * 8 < nb:
            self._partials = torch.zeros(nb // 8, dtype=torch.float64, device=self.device)
        state.copy_(self._start)
        st = self._st()
        for _ in range(int(max_iter)):
            _lib.check(self.lib.effdet_calibration_fit_step(st, scores.data_ptr(), flags.data_ptr(), iou.data_ptr(), capacity,
                                                            cursor.data_ptr(), int(threshold_index), int(self.target == 'iou'),
                                                            int(self.method == 'temperature'), state.data_ptr(),
                                                            self._partials.data_ptr(), self._partials.numel() * 8),
                       'effdet_calibration_fit_step')
        self._host, self._summary, self._fitted = None, None, True
        return self

    def finish(self):
        """ONE small device-to-host copy -> dict(a, b, iterations, halvings, converged, nll_before, nll_after, entries[, temperature]).
        Raises when the fit did not converge (separable data, such as every target equal, diverges) or a <= 0."""
        if not self._fitted and self._summary is not None:
            return dict(self._summary)
        if self._state is None:
            raise RuntimeError('nothing was fitted or loaded')
        s = dict(zip(_FIELDS, self._state.cpu().tolist()))
        out = dict(a=s['a'], b=s['b'], iterations=int(s['iterations']), halvings=int(s['halvings']), converged=bool(s['converged']),
                   nll_before=s['nll_before'], nll_after=s['nll'], entries=int(s['entries']))
        if self.method == 'temperature' and s['a'] > 0:
            out['temperature'] = 1.0 / s['a']
        if self._fitted and not out['converged']:
            raise RuntimeError('the calibration fit did not converge in %d evaluations (%d halvings, %d entries): a = %r, b = %r'
                               % (out['iterations'], out['halvings'], out['entries'], out['a'], out['b']))
        if not out['a'] > 0:
            raise RuntimeError('the fitted slope a = %r is not positive: the map would not be monotone' % (out['a'],))
        self._host, self._summary, self._fitted = (out['a'], out['b']), out, False
        return dict(out)

    # ---- apply ------------------------------------------------------------------------------------------------------------------------
    def apply(self, det, count, out=None):
        """det [B, max_det, 6] float32 on the device, count [B] int32 -> the same tensor with column 4 of the rows below `count`
        calibrated; everything else is copied.  Reads (a, b) on the device: no host synchronisation.  out: None (a new tensor) or
        a tensor like det (det itself is allowed).  Raises when nothing was fitted or loaded."""
        if not torch.is_tensor(det) or det.device.type != 'cuda' or not torch.is_tensor(count) or count.device.type != 'cuda':
            raise RuntimeError('apply() takes GPU tensors (no CPU fallback)')
        if det.dim() != 3 or det.shape[2] != 6 or det.dtype != torch.float32 or count.numel() != det.shape[0]:
            raise ValueError('det must be [B, max_det, 6] float32 and count [B]')
        if not self._fitted and self._host is None:
            raise RuntimeError('apply() before fit() or load_state_dict(): there is no (a, b) to apply')
        state = self._blocks()
        det = det.contiguous()
        count = count.to(dtype=torch.int32).contiguous()
        if out is None:
            out = torch.empty_like(det)
        elif out.shape != det.shape or out.dtype != det.dtype or out.device != det.device or not out.is_contiguous():
            raise ValueError('out must be a contiguous tensor like det')
        B, max_det, _ = det.shape
        _lib.check(self.lib.effdet_calibration_apply(self._st(), det.data_ptr(), count.data_ptr(), state.data_ptr(), B, max_det,
                                                     out.data_ptr()), 'effdet_calibration_apply')
        return out

    # ---- persistence ------------------------------------------------------------------------------------------------------------------
    def state_dict(self):
        if self._fitted:
            self.finish()
        if self._host is None:
            raise RuntimeError('nothing was fitted or loaded')
        return dict(a=float(self._host[0]), b=float(self._host[1]), method=self.method, target=self.target)

    def load_state_dict(self, sd):
        if sd['method'] not in METHODS or sd['target'] not in TARGETS:
            raise ValueError('unknown method or target in the state dict')
        a, b = float(sd['a']), float(sd['b'])
        if not a > 0 or b != b or a == float('inf') or abs(b) == float('inf'):
            raise ValueError('a must be positive and finite and b finite, got %r, %r' % (a, b))
        self.method, self.target = sd['method'], sd['target']
        self._host, self._fitted = (a, b), False
        self._summary = dict(a=a, b=b, iterations=0, halvings=0, converged=True, nll_before=float('nan'), nll_after=float('nan'),
                             entries=0)
        if self._state is not None:
            self._state.copy_(torch.tensor(_start_state(a, b), dtype=torch.float64))
        return self
