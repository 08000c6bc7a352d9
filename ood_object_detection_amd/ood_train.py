"""Energy-margin OOD training losses on the device (csrc/energy_reg.hip): a regulariser that shapes the energy of the
class head so that it separates known from unknown, forward and backward in one call over the packed [B, N, C] class logits.

    reg = EnergyRegularizer(config.num_classes, 'hinge', margin_in=-6.0, margin_out=-2.0, weight_in=0.1, weight_out=0.1)
    step = PretrainStep(model, ood_regularizer=reg)          # target['outlier']: [B] bool, the outlier-exposure images
    out = step(x, target)                                    # out['loss'] = detection loss + out['ood_loss']

    roles = anchor_roles(cls_targets, outlier_images)        # or by hand: int8 [B, N], 1 in-distribution, 0 outlier, else not counted
    loss, stats = reg(class_out, roles)

Per row z of C logits (float32, or bfloat16 widened exactly), in float32:

    energy 'logsumexp'   E = -T logsumexp(z / T)  (at T = 1 the head's own `energy`);   'joint'   E = -sum_k softplus(z_k), minus
                         `LogitOOD`'s joint_energy (the energy of a sigmoid-trained head; T must be 1)
    form 'hinge'         l_in = max(0, E - margin_in)^2,  l_out = max(0, margin_out - E)^2      (energy-bounded, Liu et al. 2020)
    form 'logistic'      s = w (-E) + b,  l_in = softplus(-s),  l_out = softplus(s)              (the uncertainty loss of VOS, Du et al.
                         2022, with the learnable scalar map phi = (w, b))
    loss = weight_in mean_in l + weight_out mean_out l;  an outlier row counts only when max z >= min_max_logit

The energy and the gradient to the logits are float32; the terms of the sums over rows (l and its derivative to s) are evaluated in
float64 from the row's float32 results (the hinge's max(0, .); the maximum and the sum of exponentials of the log-sum-exp, whose last
three operations are repeated in float64; the joint energy) and added in float64 in a fixed order.  The counts stay on the device,
nothing synchronises with the host, everything can be captured in a graph and gives the same bits every run.  There is no CPU
fallback.

`virtual_outlier_loss` is the regulariser without outlier images (VOS): the outlier side is rows that `ood_synth.OutlierSynthesizer`
draws in the input space of the class head's last pointwise map, pushed through that map:

    synth = OutlierSynthesizer(config.fpn_channels, config.num_classes, num_anchors)
    step = PretrainStep(model, ood_regularizer=EnergyRegularizer(config.num_classes, 'logistic'), outlier_synthesizer=synth)"""
import numpy as np
import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _lib

MAX_CLASSES = 1024
MAX_ROWS = 1 << 27
FORMS = ('hinge', 'logistic')
ENERGIES = ('logsumexp', 'joint')
STAT_KEYS = ('n_in', 'n_out', 'mean_l_in', 'mean_l_out', 'mean_energy_in', 'mean_energy_out', 'active_in', 'active_out')


class _EnergyRegFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, phi, roles, reg, return_energy):
        lib = _lib.load()
        B, N, C = logits.shape
        dev = logits.device
        z = logits.contiguous()
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        stats = torch.empty(8, dtype=torch.float64, device=dev)
        g_phi = torch.empty(2, dtype=torch.float32, device=dev)
        energy = torch.empty(B, N, dtype=torch.float32, device=dev) if return_energy else None
        g_z = torch.empty_like(z) if ctx.needs_input_grad[0] else None
        nws = lib.effdet_energy_reg_workspace_bytes(B * N)
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)
        p = phi.detach().contiguous() if phi is not None else None
        st = torch.cuda.current_stream(dev).cuda_stream
        ptr = lambda t: None if t is None else t.data_ptr()
        _lib.check(lib.effdet_energy_reg(st, 0 if z.dtype == torch.float32 else 1, z.data_ptr(), roles.data_ptr(), B, N, C,
                                         FORMS.index(reg.form), ENERGIES.index(reg.energy), reg.temperature, reg.margin_in or 0.0,
                                         reg.margin_out or 0.0, reg.weight_in, reg.weight_out, int(reg.min_max_logit is not None),
                                         float(reg.min_max_logit or 0.0), ptr(p), loss.data_ptr(), stats.data_ptr(), ptr(energy),
                                         ptr(g_z), g_phi.data_ptr(), ws.data_ptr(), nws), 'effdet_energy_reg')
        ctx.save_for_backward(g_z, g_phi)
        ctx.has_phi = phi is not None
        if energy is None:
            energy = torch.empty(0, dtype=torch.float32, device=dev)
        ctx.mark_non_differentiable(stats, energy)
        return loss[0].clone(), stats, energy

    @staticmethod
    @once_differentiable                                        # a second-order backward is not built: differentiating twice raises
    def backward(ctx, g_loss, _g_stats, _g_energy):
        g_z, g_phi = ctx.saved_tensors
        gz = None if g_z is None else g_z * g_loss.to(g_z.dtype)
        gp = g_phi * g_loss.to(g_phi.dtype) if ctx.has_phi and ctx.needs_input_grad[1] else None
        return gz, gp, None, None, None


class EnergyRegularizer(nn.Module):
    """The energy-margin loss of rows of class logits (module docstring).  1 <= num_classes <= 1024.  form 'hinge' needs both margins
    (they depend on num_classes and on the head: there is no default); form 'logistic' owns phi = (w, b), initialised to (1, 0).
    forward(cls_outputs, roles, return_energy=False) -> (loss, stats): cls_outputs is the head's per-level [B, A * C, H, W] list or a
    packed [B, N, C] tensor (float32 or bfloat16, GPU), roles int8 [B, N]; stats is a dict of device tensors: n_in, n_out, active_in,
    active_out (int64; rows with a positive hinge), mean_l_in / out, mean_energy_in / out (float64) and, with return_energy, energy
    [B, N] float32 (0 where the row does not count)."""

    def __init__(self, num_classes, form, energy='logsumexp', temperature=1.0, margin_in=None, margin_out=None, weight_in=1.0,
                 weight_out=1.0, min_max_logit=None):
        super().__init__()
        self.num_classes = int(num_classes)
        if not 1 <= self.num_classes <= MAX_CLASSES:
            raise ValueError('num_classes must lie in [1, %d], got %d' % (MAX_CLASSES, self.num_classes))
        if form not in FORMS:
            raise ValueError('form must be one of %r, got %r' % (FORMS, form))
        if energy not in ENERGIES:
            raise ValueError('energy must be one of %r, got %r' % (ENERGIES, energy))
        self.form, self.energy, self.temperature = form, energy, float(temperature)
        if not (self.temperature > 0.0 and np.isfinite(self.temperature)):
            raise ValueError('temperature must be > 0, got %r' % (temperature,))
        if energy == 'joint' and self.temperature != 1.0:
            raise ValueError("energy 'joint' has no temperature: it must be 1, got %r" % (temperature,))
        if form == 'hinge':
            if margin_in is None or margin_out is None:
                raise ValueError("form 'hinge' needs margin_in and margin_out (they depend on num_classes and on the head)")
            if not (np.isfinite(float(margin_in)) and np.isfinite(float(margin_out))):
                raise ValueError('the margins must be finite')
        self.margin_in = None if margin_in is None else float(margin_in)
        self.margin_out = None if margin_out is None else float(margin_out)
        self.weight_in, self.weight_out = float(weight_in), float(weight_out)
        if not (np.isfinite(self.weight_in) and np.isfinite(self.weight_out)):
            raise ValueError('the weights must be finite')
        if min_max_logit is not None and not np.isfinite(float(min_max_logit)):
            raise ValueError('min_max_logit must be finite or None')
        self.min_max_logit = None if min_max_logit is None else float(min_max_logit)
        self.phi = nn.Parameter(torch.tensor([1.0, 0.0])) if form == 'logistic' else None

    def _logits(self, cls_outputs):
        C = self.num_classes
        msg = 'cls_outputs: a [B, N, %d] tensor or a list of [B, A * %d, H, W] tensors' % (C, C)
        if not torch.is_tensor(cls_outputs):
            from .effdet.loss import _pack
            outs = list(cls_outputs)
            if not outs or any(not torch.is_tensor(t) or t.dim() != 4 or t.shape[1] % C for t in outs):
                raise ValueError(msg)
            if outs[0].device.type != 'cuda':
                raise RuntimeError('EnergyRegularizer: logits must be GPU tensors (no CPU fallback)')
            cls_outputs = _pack(outs, C)
        if cls_outputs.device.type != 'cuda':
            raise RuntimeError('EnergyRegularizer: logits must be GPU tensors (no CPU fallback)')
        if cls_outputs.dim() != 3 or cls_outputs.shape[2] != C:
            raise ValueError(msg)
        if cls_outputs.dtype not in (torch.float32, torch.bfloat16):
            raise RuntimeError('logits must be float32 or bfloat16')
        B, N = cls_outputs.shape[0], cls_outputs.shape[1]
        if B < 1 or N < 1 or B * N > MAX_ROWS:
            raise ValueError('B >= 1, N >= 1 and B * N <= 2^27')
        return cls_outputs

    def forward(self, cls_outputs, roles, return_energy=False):
        logits = self._logits(cls_outputs)
        B, N = logits.shape[0], logits.shape[1]
        if not torch.is_tensor(roles) or roles.dtype != torch.int8:
            raise ValueError('roles must be an int8 tensor (anchor_roles)')
        if tuple(roles.shape) != (B, N):
            raise ValueError('roles must be [%d, %d], got %s' % (B, N, tuple(roles.shape)))
        if roles.device != logits.device:
            raise RuntimeError('roles must live on the device of the logits')
        phi = self.phi
        if phi is not None and (phi.device != logits.device or phi.dtype != torch.float32):
            raise RuntimeError('phi must be a float32 tensor on the device of the logits')
        loss, stats, energy = _EnergyRegFn.apply(logits, phi, roles.contiguous(), self, bool(return_energy))
        out = {k: (stats[i].to(torch.int64) if k.startswith(('n_', 'active_')) else stats[i]) for i, k in enumerate(STAT_KEYS)}
        if return_energy:
            out['energy'] = energy
        return loss, out


def anchor_roles(cls_targets, outlier_images, background='none'):
    """The role of every anchor for `EnergyRegularizer`, int8 [B, N]: plain torch, glue the size of the labels, on whatever device
    they live on.  cls_targets: the labeler's per-level [B, H, W, A] list or packed [B, N] (class >= 0 positive, -1 background, -2
    ignore); outlier_images: [B] bool.  In an image that is not an outlier image the positive anchors get 1; in an outlier image every
    anchor that is not ignored gets 0 (also one that carries a label); with background='outlier' the background anchors of the
    in-distribution images get 0 too (`min_max_logit` then picks the confident ones); everything else -1."""
    if background not in ('none', 'outlier'):
        raise ValueError("background must be 'none' or 'outlier', got %r" % (background,))
    if not torch.is_tensor(cls_targets):
        from .effdet.loss import _pack_targets
        cls_targets = _pack_targets(list(cls_targets), 0)
    if cls_targets.dim() != 2:
        raise ValueError('cls_targets: a [B, N] tensor or the per-level list')
    B = cls_targets.shape[0]
    if not torch.is_tensor(outlier_images) or outlier_images.dtype != torch.bool or tuple(outlier_images.shape) != (B,):
        raise ValueError('outlier_images must be a [%d] bool tensor' % B)
    out_img = outlier_images.to(cls_targets.device)[:, None]
    one = (~out_img) & (cls_targets >= 0)
    zero = out_img & (cls_targets != -2)
    if background == 'outlier':
        zero = zero | ((~out_img) & (cls_targets == -1))
    # (masks and one subtraction: no index lists, so nothing here waits for the device)
    return (one.to(torch.int8) * 2 + zero.to(torch.int8) - 1).contiguous()        # 1, 0, or -1 (the two masks never overlap)


VIRTUAL_KEYS = ('n_virtual', 'mean_l_virtual', 'mean_energy_virtual')


def virtual_outlier_loss(reg, class_out, roles, synth, weight, bias, sample=None):
    """The regulariser on the real logits plus the regulariser on the logits of virtual outliers (VOS, Du et al. 2022): rows drawn by
    `ood_synth.OutlierSynthesizer` in the input space of the class head's last pointwise map and pushed through that map,

        virtual logits = meta_ops.Linear(rows [n * k, F], weight [A * C, F], bias [A * C])  viewed as [1, n * k * A, C],

    every virtual row's role (0, or -1 for a class that was not valid at the last fit) repeated for its A anchors.
    -> (reg(class_out, roles)[0] + reg(virtual logits, virtual roles)[0], stats): the two sides of a call have separate means, so
    with real roles in {1, -1} this is one call over the concatenation.  stats: the real call's, plus n_virtual, mean_l_virtual,
    mean_energy_virtual (the outlier side of the virtual call).  The sampled rows are constants, as in VOS: the virtual side's gradient
    reaches weight, bias and phi only.  weight: [A * C, F] or the conv's [A * C, F, 1, 1]; sample: a dict `synth.sample()` returned,
    None: one is drawn (the draw counter advances)."""
    from .effdet import meta_ops
    C = reg.num_classes
    if synth.C != C:
        raise ValueError('the sampler has %d classes, the regulariser %d' % (synth.C, C))
    if weight.dim() not in (2, 4) or weight.shape[1] != synth.F or weight.shape[0] % C or weight.numel() != weight.shape[0] * synth.F:
        raise ValueError('weight must be [A * %d, %d] or [A * %d, %d, 1, 1]' % (C, synth.F, C, synth.F))
    if weight.device.type != 'cuda':
        raise RuntimeError('virtual_outlier_loss: weight must be a GPU tensor (no CPU fallback)')
    A = weight.shape[0] // C
    if bias is not None and tuple(bias.shape) != (A * C,):
        raise ValueError('bias must be [%d]' % (A * C))
    loss, stats = reg(class_out, roles)
    s = synth.sample() if sample is None else sample
    rows = s['rows'].detach()
    m = rows.shape[0] * rows.shape[1]
    v_logits = meta_ops.Linear.apply(rows.view(m, synth.F), weight.view(A * C, synth.F), bias).view(1, m * A, C)
    v_roles = s['roles'].view(m, 1).expand(m, A).reshape(1, m * A)
    v_loss, v_stats = reg(v_logits, v_roles)
    stats = dict(stats, n_virtual=v_stats['n_out'], mean_l_virtual=v_stats['mean_l_out'], mean_energy_virtual=v_stats['mean_energy_out'])
    return loss + v_loss, stats
