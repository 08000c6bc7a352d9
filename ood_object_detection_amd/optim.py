"""Optimizer half of the reference's pretrain step (pretrain.py:272-276): `clip_grad_norm_(params, 10.)` followed by
`torch.optim.Adam(lr=1e-3).step()`, as two HIP launches over ONE flat float32 buffer.

`FlatAdam` re-points the parameters (and their `.grad`s) at slices of flat buffers, so that
* the gradient exchange of data-parallel training is a single RCCL all-reduce of `flat_grad` (15.6 MB for d0 - the
  few-large-messages shape a point-to-point xGMI fabric wants; `sharding.allreduce_gradients` handles the general case),
* the squared-norm reduction and the fused clip + Adam update touch every byte exactly once.
Parameters must be float32 GPU tensors (the pretrain step keeps fp32 master weights)."""
import torch

from . import _lib


class FlatAdam(object):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=10.0):
        self.params = [p for p in params if p.requires_grad]
        if not self.params:
            raise ValueError('no trainable parameters')
        dev = self.params[0].device
        for p in self.params:
            if p.device != dev or p.dtype != torch.float32 or dev.type != 'cuda':
                raise RuntimeError('FlatAdam needs float32 parameters on one GPU (no CPU fallback)')
        self.lib = _lib.load()
        self.lr, self.betas, self.eps, self.max_grad_norm = float(lr), (float(betas[0]), float(betas[1])), float(eps), max_grad_norm
        # every parameter starts on a 64-byte boundary of the flat buffers (16-byte vector loads of the kernels that read
        # the weights in place); the padding stays zero: zero gradient, zero moments, zero update
        n = sum(self._padded(p.numel()) for p in self.params)
        self.flat_param = torch.zeros(n, dtype=torch.float32, device=dev)
        self.flat_grad = torch.zeros(n, dtype=torch.float32, device=dev)
        self.exp_avg = torch.zeros(n, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(n, dtype=torch.float32, device=dev)
        off = 0
        with torch.no_grad():
            for p in self.params:
                k = p.numel()
                self.flat_param[off:off + k].copy_(p.reshape(-1))
                p.data = self.flat_param[off:off + k].view(p.shape)          # parameters now alias the flat buffer
                p.grad = self.flat_grad[off:off + k].view(p.shape)           # autograd accumulates in place
                off += self._padded(k)
        self._ws = torch.empty(int(self.lib.effdet_sqnorm_workspace_floats()), dtype=torch.float32, device=dev)
        self._sq = torch.zeros(1, dtype=torch.float32, device=dev)
        self._bc = torch.ones(2, dtype=torch.float32, device=dev)      # device copy of Adam's bias corrections (captured steps)
        self.steps = 0

    @staticmethod
    def _padded(k):
        return (k + 15) // 16 * 16

    def zero_grad(self):
        self.flat_grad.zero_()

    def grad_norm(self):
        """Total gradient L2 norm (what clip_grad_norm_ returns), as a 0-d GPU tensor."""
        st = torch.cuda.current_stream(self.flat_grad.device).cuda_stream
        _lib.check(self.lib.effdet_sqnorm(st, self.flat_grad.data_ptr(), self.flat_grad.numel(), self._ws.data_ptr(),
                                          self._sq.data_ptr(), 0), 'effdet_sqnorm')
        return self._sq.sqrt()[0]

    def step(self):
        """clip_grad_norm_(max_grad_norm) + Adam; returns the pre-clip gradient norm (0-d GPU tensor) or None."""
        st = torch.cuda.current_stream(self.flat_grad.device).cuda_stream
        norm = None
        if self.max_grad_norm is not None:
            norm = self.grad_norm()
        self.steps += 1
        _lib.check(self.lib.effdet_adam_clip_step(
            st, self.flat_param.data_ptr(), self.flat_grad.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(),
            self.flat_param.numel(), self.lr, self.betas[0], self.betas[1], self.eps, self.steps,
            float(self.max_grad_norm or 0.0), self._sq.data_ptr() if self.max_grad_norm is not None else None), 'effdet_adam_clip_step')
        return norm

    # ---- hipGraph-friendly variant: nothing the launches depend on lives in host scalars that change per step ----------
    def advance(self):
        """Eagerly, before replaying a captured `step_captured`: count the step and refresh the device bias corrections."""
        import math
        import struct
        self.steps += 1
        # the same arithmetic as effdet_adam_clip_step's host side: the betas arrive there as C floats, powers in double
        b1, b2 = (struct.unpack('f', struct.pack('f', b))[0] for b in self.betas)
        bc = torch.tensor([1.0 - b1 ** self.steps, math.sqrt(1.0 - b2 ** self.steps)], dtype=torch.float32)
        self._bc.copy_(bc)

    def step_captured(self):
        """The launches of `step()` with the bias corrections read from device memory (capturable; call `advance()` first)."""
        st = torch.cuda.current_stream(self.flat_grad.device).cuda_stream
        norm = None
        if self.max_grad_norm is not None:
            norm = self.grad_norm()
        _lib.check(self.lib.effdet_adam_clip_step_dev(
            st, self.flat_param.data_ptr(), self.flat_grad.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(),
            self.flat_param.numel(), self.lr, self.betas[0], self.betas[1], self.eps, self._bc.data_ptr(),
            float(self.max_grad_norm or 0.0), self._sq.data_ptr() if self.max_grad_norm is not None else None), 'effdet_adam_clip_step_dev')
        return norm


# =====================================================================================================================
# Grouped optimizer: what the reference scripts ask of `meta_optimizer` beyond one Adam over everything
#   pretrain.py:179-187, :279-281   Adam with parameter groups (BiFPN at lr 0 until iteration 201), or Nesterov SGD
#   infer.py:259-286, :803-804      four groups, two separate clip_grad_norm_ calls (one covering parameters in no group)
# Parameters with `grad is None` are skipped by torch (moments do not decay, `step` does not advance): here the caller names
# the parameters that received a gradient (`step(present=...)`).  Kernels: csrc/group_optim.hip (three launches per step).
# =====================================================================================================================
PIECE_FLOATS = 2048          # effdet_group_piece_floats(): floats of one workgroup's piece (checked when the library loads)
_ALIGN = 16                  # floats: every segment starts on a 64-byte boundary and is padded to one
_GROUP_ROW = 16              # 4-byte words of a group's row in the device table


def membership(n, index_lists, what='group'):
    """index_lists[k] = indices (into n tensors) of group / domain k  ->  per-tensor k, or -1.  A tensor listed twice raises."""
    of = [-1] * n
    for k, idx in enumerate(index_lists):
        for i in idx:
            if not 0 <= i < n:
                raise ValueError('%s %d names tensor %d of %d' % (what, k, i, n))
            if of[i] == k:
                raise ValueError('some parameters appear more than once in %s %d' % (what, k))
            if of[i] != -1:
                raise ValueError('some parameters appear in more than one %s' % what)
            of[i] = k
    return of


def plan_layout(numels, group_of, domain_of, piece=PIECE_FLOATS):
    """Where every tensor goes in the flat buffers.  Pure function: no tensors, no GPU.

    numels[i]: elements of tensor i (a 0-d tensor has 1); group_of[i] / domain_of[i]: its group / clip domain, -1 or None for none
    (a tensor in neither is an error).  Segments are ordered domain after domain, then those in no domain; inside each the order of
    `numels` is kept - so a clip domain is ONE contiguous range, and a partial sum of the norm pass never straddles domains.
    Every segment starts on a 64-byte boundary and is padded to one.  Returns a dict:
      order [n]            tensor indices in buffer order (position in `order` = segment number of the device tables)
      offsets, padded [n]  per tensor i: first float and padded length
      total                floats of a flat buffer
      domain_ranges        per domain (first float, end float)
      pieces [P][4], n_norm_pieces, seg_group [n], dom_ranges [D+1][4]   the int32 tables of effdet_group_step"""
    import numpy as np
    n = len(numels)
    if n == 0:
        raise ValueError('no tensors')
    if len(group_of) != n or len(domain_of) != n:
        raise ValueError('group_of / domain_of need one entry per tensor')
    grp = [-1 if g is None else int(g) for g in group_of]
    dom = [-1 if d is None else int(d) for d in domain_of]
    if piece <= 0 or piece % _ALIGN:
        raise ValueError('piece must be a positive multiple of %d' % _ALIGN)
    for i in range(n):
        if int(numels[i]) < 1:
            raise ValueError('tensor %d is empty' % i)
        if grp[i] < -1 or dom[i] < -1:
            raise ValueError('negative group / domain')
        if grp[i] == -1 and dom[i] == -1:
            raise ValueError('tensor %d is in no group and in no clip domain' % i)
    n_dom = max(dom) + 1
    order = [i for d in list(range(n_dom)) + [-1] for i in range(n) if dom[i] == d]
    offsets, padded = [0] * n, [0] * n
    pieces, seg_group = [], []
    dom_ranges = [[0, 0, 0, 0] for _ in range(n_dom + 1)]
    domain_ranges = [[0, 0] for _ in range(n_dom)]
    off = 0
    cur = None
    for s, i in enumerate(order):
        d = dom[i] if dom[i] >= 0 else n_dom
        if d != cur:                                         # a new domain begins (domains without tensors keep empty ranges)
            for e in range((-1 if cur is None else cur) + 1, d + 1):
                dom_ranges[e] = [len(pieces), len(pieces), s, s]
                if e < n_dom:
                    domain_ranges[e] = [off, off]
            cur = d
        k = (int(numels[i]) + _ALIGN - 1) // _ALIGN * _ALIGN
        offsets[i], padded[i] = off, k
        for a in range(0, k, piece):
            pieces.append([(off + a) // 4, min(piece, k - a) // 4, s, 0])
        seg_group.append(grp[i])
        off += k
        dom_ranges[d][1], dom_ranges[d][3] = len(pieces), s + 1
        if d < n_dom:
            domain_ranges[d][1] = off
    for e in range((-1 if cur is None else cur) + 1, n_dom + 1):
        dom_ranges[e] = [len(pieces), len(pieces), n, n]
    if off // 4 >= 2 ** 31:
        raise ValueError('flat buffer too large for 32-bit piece offsets')
    return {'order': order, 'offsets': offsets, 'padded': padded, 'total': off,
            'domain_ranges': [tuple(r) for r in domain_ranges],
            'pieces': np.asarray(pieces, dtype=np.int32).reshape(-1, 4), 'n_norm_pieces': dom_ranges[n_dom][0] if n_dom else 0,
            'seg_group': np.asarray(seg_group, dtype=np.int32), 'dom_ranges': np.asarray(dom_ranges, dtype=np.int32).reshape(-1, 4)}


def _param_list(params):
    """a tensor, a module, or an iterable of tensors -> list of tensors"""
    if isinstance(params, torch.Tensor):
        return [params]
    if isinstance(params, torch.nn.Module):
        return list(params.parameters())
    return list(params)


_ADAM_KEYS = ('lr', 'betas', 'eps', 'weight_decay')
_SGD_KEYS = ('lr', 'momentum', 'nesterov', 'weight_decay')
_NOT_BUILT = (('amsgrad', False), ('maximize', False), ('dampening', 0), ('decoupled_weight_decay', False))


class GroupedOptimizer(object):
    """torch.optim.Adam / torch.optim.SGD with parameter groups plus clip_grad_norm_ per clip domain, on flat float32 buffers.

        GroupedOptimizer(param_groups, optim='adam'|'sgd', lr=, betas=, eps=, momentum=, nesterov=, weight_decay=, clip_domains=None)

    `param_groups`: torch's list of dicts ({'params': ..., optional overrides}) or an iterable of parameters (one group).
    `clip_domains`: list of {'params': ..., 'max_norm': ...}; each is one clip_grad_norm_ call with a coefficient of its own.  A
    parameter may be in a domain and in no group (it counts towards the norm and is never updated) or in a group and in no domain
    (unclipped).  Like FlatAdam, the parameters and their `.grad`s become views of `flat_param` / `flat_grad`.
    `param_groups` stays a list of live dicts: `opt.param_groups[1]['lr'] = x` takes effect at the next step."""

    def __init__(self, param_groups, optim='adam', lr=1e-3, betas=(0.9, 0.999), eps=1e-8, momentum=0.0, nesterov=False,
                 weight_decay=0.0, clip_domains=None, **not_built):
        import numpy as np
        if optim not in ('adam', 'sgd'):
            raise ValueError("optim must be 'adam' or 'sgd'")
        self.kind = 0 if optim == 'adam' else 1
        self.optim = optim
        for k in not_built:
            if k not in dict(_NOT_BUILT):
                raise TypeError('unexpected argument %r' % k)
        param_groups = list(param_groups)
        if not param_groups:
            raise ValueError('optimizer got an empty parameter list')
        if not isinstance(param_groups[0], dict):
            param_groups = [{'params': param_groups}]
        defaults = {'lr': lr, 'weight_decay': weight_decay}
        defaults.update({'betas': betas, 'eps': eps} if self.kind == 0 else {'momentum': momentum, 'nesterov': nesterov})
        groups = []
        for g in param_groups:
            g = dict(g)
            g['params'] = _param_list(g['params'])
            for k, v in defaults.items():
                g.setdefault(k, v)
            for k, off in _NOT_BUILT:
                if g.pop(k, not_built.get(k, off)) != off:
                    raise NotImplementedError('%s is not built' % k)
            self._check_group(g)
            groups.append(g)
        domains = []
        for d in (clip_domains or []):
            d = dict(d)
            d['params'] = _param_list(d['params'])
            d['max_norm'] = float(d['max_norm'])
            domains.append(d)
        # one list of distinct tensors: the groups' parameters first, in torch's state_dict numbering, then those only clipped
        params, index = [], {}
        for lst in [g['params'] for g in groups] + [d['params'] for d in domains]:
            for p in lst:
                if id(p) not in index:
                    index[id(p)] = len(params)
                    params.append(p)
        if not params:
            raise ValueError('no parameters')
        self.n_group_params = sum(len(g['params']) for g in groups)
        group_of = membership(len(params), [[index[id(p)] for p in g['params']] for g in groups], 'parameter group')
        domain_of = membership(len(params), [[index[id(p)] for p in d['params']] for d in domains], 'clip domain')
        dev = params[0].device
        self._check_params(params, dev)
        self.lib = self._load_lib()
        if int(self.lib.effdet_group_piece_floats()) != PIECE_FLOATS:
            raise RuntimeError('libeffdet_hip.so was built with another piece size')
        # ---- nothing above changed the caller's tensors; from here on nothing raises ------------------------------------------
        self.params, self.param_groups, self.clip_domains, self.device = params, groups, domains, dev
        self._index = index
        lay = self.layout = plan_layout([max(1, p.numel()) for p in params], group_of, domain_of)
        self._seg_of = [0] * len(params)                      # tensor index -> segment number
        for s, i in enumerate(lay['order']):
            self._seg_of[i] = s
        n = lay['total']
        self.flat_param = torch.zeros(n, dtype=torch.float32, device=dev)
        self.flat_grad = torch.zeros(n, dtype=torch.float32, device=dev)
        self.state1 = torch.zeros(n, dtype=torch.float32, device=dev)                  # exp_avg / momentum_buffer
        self.state2 = torch.zeros(n, dtype=torch.float32, device=dev) if self.kind == 0 else None      # exp_avg_sq
        with torch.no_grad():
            for i, p in enumerate(params):
                off, k = lay['offsets'][i], p.numel()
                self.flat_param[off:off + k].copy_(p.reshape(-1))
                p.data = self.flat_param[off:off + k].view(p.shape)
                if p.requires_grad:
                    p.grad = self.flat_grad[off:off + k].view(p.shape)
        self.n_seg, self.n_dom, self.n_groups = len(params), len(domains), len(groups)
        self._pieces = torch.from_numpy(lay['pieces']).to(dev)
        self._seg_group = torch.from_numpy(lay['seg_group']).to(dev)
        self._dom_ranges = torch.from_numpy(lay['dom_ranges']).to(dev)
        self._step = torch.zeros(self.n_seg, dtype=torch.int32, device=dev)
        self._seg_const = torch.zeros(self.n_seg * 4, dtype=torch.float32, device=dev)
        self._partial = torch.zeros(max(1, lay['n_norm_pieces']), dtype=torch.float32, device=dev)
        self._norms = torch.zeros(max(1, self.n_dom), dtype=torch.float32, device=dev)
        # everything the host may change between steps goes through ONE pinned buffer (see effdet_hip.h for the layout)
        words = self.n_groups * _GROUP_ROW + self.n_dom + self.n_seg
        self._slots = [[self._staging(words), None], [self._staging(words), None]]     # two staging buffers used in turn: [words, event after its upload]
        self._slot = 0
        self._pinned = self._slots[0][0]
        self._host = self._pinned.numpy()
        self._dyn = torch.zeros(words, dtype=torch.int32, device=dev)
        self._uploaded = None                                 # the words last uploaded (None: never)
        self._frozen = np.asarray([0 if params[i].requires_grad else 1 for i in lay['order']], dtype=np.int32)
        self._present = np.ones(self.n_seg, dtype=np.int32)
        self.refresh()

    # ---- what ties the class to a GPU (tools/simt_model/run_group_optim.py overrides these to run the kernels on its CPU model) ---
    def _check_params(self, params, dev):
        for p in params:
            if not isinstance(p, torch.Tensor) or p.device != dev or p.dtype != torch.float32 or dev.type != 'cuda':
                raise RuntimeError('GroupedOptimizer needs float32 parameters on one GPU (no CPU fallback)')

    def _load_lib(self):
        return _lib.load()

    def _staging(self, words):
        return torch.zeros(words, dtype=torch.int32).pin_memory()

    def _stream(self):
        """-> (stream handle, is it capturing)"""
        return torch.cuda.current_stream(self.device).cuda_stream, torch.cuda.is_current_stream_capturing()

    def _upload(self):
        """One non-blocking copy from the staging buffer that was not used by the previous upload.  Its words may be rewritten
        once the upload before that one has read them: the event wait below is on a copy two uploads back, so the host runs
        ahead of the device by up to two changed tables before it ever waits."""
        self._slot ^= 1
        slot = self._slots[self._slot]
        if slot[1] is not None:
            slot[1].synchronize()
        self._pinned = slot[0]
        self._host = self._pinned.numpy()
        self._host[:] = self._uploaded
        self._dyn.copy_(self._pinned, non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record(torch.cuda.current_stream(self.device))

    # ---- host side of the device tables -----------------------------------------------------------------------------------
    def _check_group(self, g):
        if not g['lr'] >= 0.0:
            raise ValueError('invalid learning rate')
        if not g['weight_decay'] >= 0.0:
            raise ValueError('invalid weight_decay')
        if self.kind == 0:
            b1, b2 = g['betas']
            if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
                raise ValueError('invalid betas')
            if not g['eps'] > 0.0:                            # eps = 0 would turn the zero padding into 0 / 0
                raise ValueError('eps must be positive')
        else:
            if not g['momentum'] >= 0.0:
                raise ValueError('invalid momentum')
            if g['nesterov'] and g['momentum'] <= 0:
                raise ValueError('Nesterov momentum requires a momentum and zero dampening')

    def _host_words(self):
        import numpy as np
        w = np.zeros(self._host.shape[0], dtype=np.int32)
        for k, g in enumerate(self.param_groups):
            self._check_group(g)
            for key, off in _NOT_BUILT:
                if g.get(key, off) != off:
                    raise NotImplementedError('%s is not built' % key)
            row = w[k * _GROUP_ROW:(k + 1) * _GROUP_ROW]
            d, f = row[:6].view(np.float64), row[6:12].view(np.float32)
            d[0] = float(g['lr'])
            if self.kind == 0:
                b1, b2 = float(g['betas'][0]), float(g['betas'][1])
                d[1], d[2] = b1, b2
                f[0], f[1], f[2], f[3], f[4] = g['weight_decay'], g['eps'], 1.0 - b1, b2, 1.0 - b2      # rounded once, as torch's scalars
            else:
                f[0], f[5] = g['weight_decay'], g['momentum']
                row[12] = 1 if g['nesterov'] else 0
        base = self.n_groups * _GROUP_ROW
        w[base:base + self.n_dom].view(np.float32)[:] = [float(d['max_norm']) for d in self.clip_domains]
        w[base + self.n_dom:] = self._present & (1 - self._frozen)
        return w

    def set_present(self, present=None):
        """Name the parameters (tensors and / or modules) that received a gradient in this accumulation window; the others are
        treated as torch treats `grad is None`.  None: all.  Takes effect at the next `refresh()` (`step()` calls it when eager)."""
        if present is None:
            self._present[:] = 1
            return
        self._present[:] = 0
        for item in present:
            for p in _param_list(item):
                i = self._index.get(id(p))
                if i is not None:
                    self._present[self._seg_of[i]] = 1

    def refresh(self):
        """Upload learning rates, hyper-parameters, max norms and the present mask if they differ from what the device has
        (one non-blocking copy from pinned memory).  Before each replay of a captured `step()`; `step()` calls it when eager."""
        import numpy as np
        w = self._host_words()
        if self._uploaded is not None and np.array_equal(w, self._uploaded):
            return False
        self._uploaded = w
        self._upload()
        return True

    # ---- FlatAdam's surface -------------------------------------------------------------------------------------------------
    def zero_grad(self):
        self.flat_grad.zero_()

    def _table_args(self):
        lay = self.layout
        return (self._pieces.data_ptr(), int(lay['pieces'].shape[0]), int(lay['n_norm_pieces']), self._seg_group.data_ptr(), self.n_seg,
                self._dom_ranges.data_ptr(), self.n_dom, self._dyn.data_ptr(), self.n_groups)

    def grad_norm(self):
        """The pre-clip gradient norm of every clip domain (what each clip_grad_norm_ returns): 1-d GPU tensor.  Nothing advances."""
        if self.n_dom == 0:
            return torch.zeros(0, dtype=torch.float32, device=self.device)
        st, capturing = self._stream()
        if not capturing:
            self.refresh()
        _lib.check(self.lib.effdet_group_norms(st, self.flat_grad.data_ptr(), self.flat_grad.numel(), *self._table_args(),
                                               self._partial.data_ptr(), self._norms.data_ptr()), 'effdet_group_norms')
        return self._norms.clone()

    def step(self, present=None):
        """Per-domain clip + Adam / SGD; returns the pre-clip norms (1-d GPU tensor, one per domain; `.sum()` is infer.py's logged
        figure).  `present`: see `set_present`; an eager step always sets the mask, so `None` means all parameters whatever an
        earlier `set_present()` said.  Under graph capture only the three launches are recorded: the present mask and the
        host tables are left alone, the caller calls `set_present()` / `refresh()` before each replay, and passing `present`
        raises."""
        st, capturing = self._stream()
        if capturing:
            if present is not None:
                raise RuntimeError('step(present=...) while capturing: call set_present() and refresh() before each replay instead')
        else:
            self.set_present(present)
            self.refresh()
        _lib.check(self.lib.effdet_group_step(
            st, self.kind, self.flat_param.data_ptr(), self.flat_grad.data_ptr(), self.state1.data_ptr(),
            self.state2.data_ptr() if self.state2 is not None else None, self.flat_param.numel(), *self._table_args(),
            self._step.data_ptr(), self._seg_const.data_ptr(), self._partial.data_ptr(), self._norms.data_ptr()), 'effdet_group_step')
        return self._norms[:self.n_dom].clone()

    # ---- torch's state_dict layout ----------------------------------------------------------------------------------------------
    def _view(self, flat, i):
        off = self.layout['offsets'][i]
        return flat[off:off + self.params[i].numel()].view(self.params[i].shape)

    def _torch_group(self, g, idx):
        if self.kind == 0:
            out = {'lr': g['lr'], 'betas': tuple(g['betas']), 'eps': g['eps'], 'weight_decay': g['weight_decay'], 'amsgrad': False,
                   'maximize': False, 'foreach': None, 'capturable': False, 'differentiable': False, 'fused': None,
                   'decoupled_weight_decay': False}
        else:
            out = {'lr': g['lr'], 'momentum': g['momentum'], 'dampening': 0, 'weight_decay': g['weight_decay'], 'nesterov': bool(g['nesterov']),
                   'maximize': False, 'foreach': None, 'differentiable': False, 'fused': None}
        for k, v in g.items():                                # keys of the caller's own travel along, as in torch
            if k != 'params':
                out.setdefault(k, v)
        out['params'] = idx
        return out

    def state_dict(self):
        """{'state': {index: ...}, 'param_groups': [...]} as torch.optim.Adam / SGD over the same parameter list would give it:
        loads into them, and theirs loads here.  Entries are absent for parameters never updated."""
        steps = self._step.cpu().tolist()
        state, groups, i = {}, [], 0
        for g in self.param_groups:
            idx = list(range(i, i + len(g['params'])))
            i += len(idx)
            groups.append(self._torch_group(g, idx))
            for j in idx:
                t = steps[self._seg_of[j]]
                if t <= 0:
                    continue
                if self.kind == 0:
                    state[j] = {'step': torch.tensor(float(t), dtype=torch.float32), 'exp_avg': self._view(self.state1, j).clone(),
                                'exp_avg_sq': self._view(self.state2, j).clone()}
                else:
                    state[j] = {'momentum_buffer': self._view(self.state1, j).clone()}
        return {'state': state, 'param_groups': groups}

    def load_state_dict(self, sd):
        import numpy as np
        sgroups = sd['param_groups']
        if len(sgroups) != len(self.param_groups):
            raise ValueError('loaded state dict has a different number of parameter groups')
        if any(len(s['params']) != len(g['params']) for s, g in zip(sgroups, self.param_groups)):
            raise ValueError("loaded state dict contains a parameter group that doesn't match the size of optimizer's group")
        keys = _ADAM_KEYS if self.kind == 0 else _SGD_KEYS
        new = []
        for s, g in zip(sgroups, self.param_groups):
            for k, off in _NOT_BUILT:
                if s.get(k, off) != off:
                    raise NotImplementedError('%s is not built' % k)
            h = dict(g)
            h.update({k: s[k] for k in keys})
            self._check_group(h)
            new.append(h)
        flat_idx = [j for s in sgroups for j in s['params']]          # saved index of our parameter number i
        steps = np.zeros(self.n_seg, dtype=np.int32)
        fresh1 = torch.zeros_like(self.state1)
        fresh2 = torch.zeros_like(self.state2) if self.kind == 0 else None
        for i, j in enumerate(flat_idx):
            st = sd['state'].get(j)
            if not st:
                continue
            if self.kind == 0:
                steps[self._seg_of[i]] = int(round(float(st['step'])))
                self._view(fresh1, i).copy_(st['exp_avg'])
                self._view(fresh2, i).copy_(st['exp_avg_sq'])
            elif st.get('momentum_buffer') is not None:
                steps[self._seg_of[i]] = 1
                self._view(fresh1, i).copy_(st['momentum_buffer'])
        for g, h in zip(self.param_groups, new):                      # the live dicts stay the same objects
            g.update({k: h[k] for k in keys})
        self.state1.copy_(fresh1)
        if self.kind == 0:
            self.state2.copy_(fresh2)
        self._step.copy_(torch.from_numpy(steps))
        self.refresh()


def script_param_groups(model, proj_net=None, learnable_lr=(), meta_lr=1e-3, train_bb=False, separate_head=False, max_norm=10.0):
    """-> (param_groups, clip_domains) as the reference scripts build them, for GroupedOptimizer.

    proj_net None: pretrain.py:181-185 - with `train_bb` backbone, BiFPN, class net, box net at `meta_lr`; without it the BiFPN
    at lr 0 (the script raises it at iteration 201, :279-281), the two heads at `meta_lr`, the backbone in no group; one clip over
    model.parameters() (:272).  With proj_net: infer.py:259-274 - predict_pars, class_pars, proj_net, learnable_lr (lr 0) with
    `separate_head` choosing the *_sep names and freezing class_pars / proj_net - and the two clips of :803-804."""
    if proj_net is None:
        if train_bb:
            groups = [{'params': list(model.backbone.parameters())}, {'params': list(model.fpn.parameters())},
                      {'params': list(model.class_net.parameters())}, {'params': list(model.box_net.parameters())}]
        else:
            groups = [{'params': list(model.fpn.parameters()), 'lr': 0.}, {'params': list(model.class_net.parameters())},
                      {'params': list(model.box_net.parameters())}]
        for g in groups:
            g.setdefault('lr', meta_lr)
        return groups, [{'params': list(model.parameters()), 'max_norm': max_norm}]
    names = ['predict_pw_sep', 'predict_pb_sep'] if separate_head else ['predict_pw', 'predict_pb']
    class_pars = [p for n, p in model.class_net.named_parameters() if n not in names]
    predict_pars = [p for n, p in model.class_net.named_parameters() if n in names]
    rest = 0. if separate_head else meta_lr
    groups = [{'params': predict_pars, 'lr': meta_lr}, {'params': class_pars, 'lr': rest},
              {'params': list(proj_net.parameters()), 'lr': rest}, {'params': list(learnable_lr), 'lr': 0.}]
    return groups, [{'params': list(proj_net.parameters()), 'max_norm': max_norm}, {'params': list(model.parameters()), 'max_norm': max_norm}]
