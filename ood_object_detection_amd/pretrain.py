"""One iteration of the reference's pretrain loop (pretrain.py:220-276) on the HIP path.

    meta_optimizer.zero_grad()
    qry_imgs = (qry_imgs.float() - imagenet_mean) / imagenet_std          pretrain.py:226   (uint8 input: effdet_normalize_u8)
    feats = model(qry_imgs, mode='bb')                                    :229
    class_out, box_out = model(feats, mode='fpn_and_head')                :232
    qry_loss, ... = loss_fn(class_out, box_out, cls_anchors, bbox_anchors, num_positives)   :233
    qry_loss.backward()                                                   :236
    clip_grad_norm_(model.parameters(), 10.); meta_optimizer.step()       :272-276

Data-parallel training (BASELINE config 5) adds ONE collective: the flat float32 gradient buffer of `FlatAdam`
(15.6 MB for d0) is all-reduced (mean) over RCCL between backward and the optimizer step - one large message, the
shape a point-to-point xGMI fabric wants.  BN stays per replica (no SyncBN in the reference).  Defaults mirror the
script's flags: Adam lr 1e-3, alpha .15, box weight 50, delta .1 (pretrain.py:57-62), backbone BN frozen in eval mode
(`freeze_bb_bn`, :168-176), BiFPN / head BN in batch-statistics mode.
"""
import torch
import torch.nn as nn

from .optim import FlatAdam


def set_bn_eval(module):
    """pretrain.py:169-171"""
    if isinstance(module, nn.modules.batchnorm._BatchNorm):
        module.eval()


class PretrainStep(object):
    def __init__(self, model, lr=1e-3, max_grad_norm=10.0, alpha=0.15, box_loss_weight=50.0, freeze_bn=False,
                 labeler=True, graph=False, graph_warmup=2, optimizer=None, ood_regularizer=None, ood_background='none',
                 outlier_synthesizer=None, synth_refresh_every=100, synth_shrinkage=0.0, vmf_head=None, vmf_weight=1.5):
        """graph=True: after `graph_warmup` eager iterations the whole iteration (zero_grad, forward, loss, backward and -
        single GPU - clip + Adam) is captured into one hipGraph and replayed; the ~5 000 launches of a step then cost one
        submission.  Shapes must stay fixed; labels are assigned eagerly and copied into the graph's static buffers.
        optimizer: an `optim.GroupedOptimizer` over (some of) the model's parameters, used in place of the FlatAdam that is
        otherwise built from `lr` / `max_grad_norm` (parameter groups, clip domains, Nesterov SGD: optim.script_param_groups);
        'grad_norm' is then its 1-d tensor of per-domain norms.
        ood_regularizer: an `ood_train.EnergyRegularizer`; target['outlier'] ([B] bool) then names the outlier-exposure images, the
        roles of the anchors are formed next to the labels (`ood_train.anchor_roles`, background=ood_background), the loss is the
        detection loss plus the regulariser's, and the returned dict gains 'ood_loss' and the regulariser's statistics.  The default
        FlatAdam then covers the model's parameters followed by the regulariser's; a caller's optimizer covers them or not.
        outlier_synthesizer: an `ood_synth.OutlierSynthesizer` (needs an ood_regularizer; VOS, Du et al. 2022).  Every step adds the
        penultimate features of the class head at the positive anchors to its statistics (no synchronisation); after every
        `synth_refresh_every` steps `fit(synth_shrinkage)` runs - the one host read, outside any graph, raising like
        `FeatureOOD.fit`; once a fit exists the regulariser's term is `ood_train.virtual_outlier_loss`, the virtual rows pushed
        through class_net.predict.conv_pw, and the returned dict gains n_virtual, mean_l_virtual and mean_energy_virtual.
        target['outlier'] is then optional (default: no outlier image).  With graph=True the steps before the first fit run
        eagerly; the capture holds the virtual side and reads a later fit from the buffers `fit` writes in place.
        vmf_head: an `ood_vmf.VMFHead` (SIREN, Du et al. 2022).  The engine's fpn-and-heads node then also returns the class tower
        (`TrainEngine.tower_output`), the head embeds it, updates its prototypes from the step's labels and adds
        `vmf_weight` times its vMF loss, whose gradient reaches the class tower and the BiFPN; the returned dict gains 'vmf_loss'
        and the head's statistics as 'vmf_m', 'vmf_skipped', ...  The default FlatAdam also covers the head's parameters."""
        from .effdet.anchors import Anchors, AnchorLabeler
        from .effdet.config import set_config_writeable
        from .effdet.loss import DetectionLoss
        self.model = model
        model.train()
        if freeze_bn:
            model.apply(set_bn_eval)
        else:
            model.backbone.apply(set_bn_eval)
        cfg = model.config
        set_config_writeable(cfg)
        cfg.alpha, cfg.box_loss_weight = alpha, box_loss_weight
        self.loss_fn = DetectionLoss(cfg)
        self._grouped = optimizer is not None
        self.ood, self.ood_background = ood_regularizer, ood_background
        self.synth, self.synth_refresh_every, self.synth_shrinkage = outlier_synthesizer, int(synth_refresh_every), float(synth_shrinkage)
        if self.synth is not None:
            if self.ood is None:
                raise ValueError('an outlier_synthesizer needs an ood_regularizer')
            if self.synth_refresh_every < 1:
                raise ValueError('synth_refresh_every must be >= 1')
            pw = model.class_net.predict.conv_pw
            if (self.synth.C, self.synth.F) != (cfg.num_classes, pw.weight.shape[1]) or pw.weight.shape[0] != self.synth.A * self.synth.C:
                raise ValueError('the outlier_synthesizer must have the class head\'s num_classes, width and anchors per cell')
        self.vmf, self.vmf_weight = vmf_head, float(vmf_weight)
        if self.vmf is not None:
            pw = model.class_net.predict.conv_pw
            if (self.vmf.C, self.vmf.F) != (cfg.num_classes, pw.weight.shape[1]) or pw.weight.shape[0] != self.vmf.A * self.vmf.C:
                raise ValueError('the vmf_head must have the class head\'s num_classes, width and anchors per cell')
        self._cap_vmf = None
        self._synth_steps = 0                   # steps since the synthesiser was given: fit after every synth_refresh_every-th
        self._synth_eager = 0                   # eager steps that ran the virtual side (one comes before a capture)
        if self._grouped:
            self.opt = optimizer
        elif self.ood is None and self.vmf is None:
            self.opt = FlatAdam(model.parameters(), lr=lr, max_grad_norm=max_grad_norm)
        else:
            extra = ([] if self.ood is None else list(self.ood.parameters())) + ([] if self.vmf is None else list(self.vmf.parameters()))
            self.opt = FlatAdam(list(model.parameters()) + extra, lr=lr, max_grad_norm=max_grad_norm)
        self.anchors = Anchors.from_config(cfg).to(model.backbone.conv_stem.weight.device)
        self.labeler = AnchorLabeler(self.anchors, cfg.num_classes, match_threshold=0.5) if labeler else None
        self.num_levels = cfg.num_levels
        self.world = 1
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            self.world = dist.get_world_size()
        self.last_allreduce_ms = 0.0
        self.graph = bool(graph)
        # the stage tables upload at the end of the first backward and at the start of the second forward (host-to-device copies,
        # which cannot be captured): at least two eager iterations before the capture
        self._graph_warmup = max(2, int(graph_warmup))
        self._calls = 0
        self._cap = None                        # (graph, optimizer graph or None, static inputs, static outputs)
        self._static_base = None
        self._cap_ood = None                    # with a regulariser: (static roles, its captured loss and statistics)

    def targets(self, target):
        """target: {'bbox': [per-image [M,4] yxyx], 'cls': [per-image [M]]} (labelled on the GPU, effdet/anchors.py:384-438)
        or the loader's pre-labelled {'label_cls_l', 'label_bbox_l', 'label_num_positives'} (effdet/bench.py:127-133)."""
        if 'label_num_positives' in target:
            return ([target['label_cls_%d' % l] for l in range(self.num_levels)],
                    [target['label_bbox_%d' % l] for l in range(self.num_levels)], target['label_num_positives'])
        if self.labeler is None:
            raise ValueError('pre-labelled targets or labeler=True needed')
        return self.labeler.batch_label_anchors(target['bbox'], target['cls'])

    def roles(self, target, cls_t):
        """with a regulariser: the int8 [B, N] role of every anchor from the labels and target['outlier'], else None"""
        if self.ood is None:
            return None
        from .ood_train import anchor_roles
        if 'outlier' not in target:
            if self.synth is None:
                raise ValueError("an ood_regularizer needs target['outlier'], a [B] bool tensor")
            return anchor_roles(cls_t, torch.zeros(cls_t[0].shape[0], dtype=torch.bool, device=cls_t[0].device), self.ood_background)
        return anchor_roles(cls_t, target['outlier'].to(cls_t[0].device), self.ood_background)

    def _ood_terms(self, class_out, cls_t, roles):
        """the regulariser's loss and statistics; with a synthesiser the positives' penultimate features join its statistics and,
        once it is fitted, the virtual outliers join the loss"""
        if self.synth is None:
            return self.ood(class_out, roles)
        self.synth.add_targets(self.model._train_engine.class_penultimate(), cls_t)
        if not self.synth.fitted:
            return self.ood(class_out, roles)
        from .ood_train import virtual_outlier_loss
        pw = self.model.class_net.predict.conv_pw
        return virtual_outlier_loss(self.ood, class_out, roles, self.synth, pw.weight, pw.bias)

    def _vmf_terms(self, cls_t):
        """with a vmf_head: its weighted loss on the differentiable class tower of the forward just run, and its statistics"""
        vmf_loss, stats = self.vmf(self.model._train_engine.class_tower, cls_t)
        return self.vmf_weight * vmf_loss, dict({'vmf_' + k: v for k, v in stats.items()}, vmf_loss=vmf_loss.detach())

    def _synth_refresh(self):
        if self.synth is not None:
            self._synth_steps += 1
            if self._synth_steps % self.synth_refresh_every == 0:
                self.synth.fit(self.synth_shrinkage)

    def detections(self, class_out, box_out):
        """pretrain.py:238-245: _post_process + generate_detections(hard NMS, no clipping) for the whole batch.
        -> det [B, 100, 6] (x1,y1,x2,y2,score,class 1-based, zero padded), count [B]"""
        from .effdet.anchors import batched_detections
        from .effdet.bench import _post_process
        cfg = self.model.config
        with torch.no_grad():
            co, bo = [t.detach() for t in class_out], [t.detach() for t in box_out]
            ct, bt, idx, cl = _post_process(co, bo, cfg.num_levels, cfg.num_classes, cfg.max_detection_points)
            B, k = idx.shape
            det, count, _ = batched_detections(ct.reshape(B, k), bt, self.anchors.boxes, idx, cl, None, None,
                                               max_det_per_image=cfg.max_det_per_image, soft_nms=False)
        return det, count

    def evaluate(self, class_out, box_out, target, evaluator):
        """pretrain.py:246-252: add the batch's detections and ground truth (target['bbox'] yxyx / target['cls'] 1-based lists)
        to a device `ObjectDetectionEvaluator` (cleared by the caller per iteration, as the script does)."""
        det, count = self.detections(class_out, box_out)
        B = det.shape[0]
        M = max(1, max(int(b.shape[0]) for b in target['bbox']))
        gtb = torch.zeros(B, M, 4, dtype=torch.float32, device=det.device)
        gtc = torch.full((B, M), -1, dtype=torch.int64, device=det.device)
        for i, (b, c) in enumerate(zip(target['bbox'], target['cls'])):
            m = int(b.shape[0])
            if m:
                gtb[i, :m] = b.to(det.device, torch.float32)
                gtc[i, :m] = c.to(det.device, torch.int64)
        evaluator.add_batch(det, count, gtb, gtc)
        return det, count

    # ---- captured iteration ---------------------------------------------------------------------------------
    def _capture(self, x, cls_t, box_t, npos, roles=None):
        model, opt = self.model, self.opt
        from .effdet.loss import _pack_targets
        sx = x.clone()
        # static targets: ONE packed tensor each when they are the labeler's views (one copy per replay instead of one per level)
        cb, bb = _pack_targets(list(cls_t), 0), _pack_targets(list(box_t), 4)
        if self.labeler is not None and cb is cls_t[0]._base and bb is box_t[0]._base:
            self._static_base = (cb.clone(), bb.clone())
            s_cls, s_box = self.labeler._unpack(*self._static_base)
        else:
            self._static_base = None
            s_cls = [t.clone() for t in cls_t]
            s_box = [t.clone() for t in box_t]
        s_np = npos.clone()
        s_roles = None if roles is None else roles.clone()
        torch.cuda.synchronize()
        g1 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g1):
            opt.zero_grad()
            feats = model(sx, mode='bb')
            class_out, box_out = model(feats, mode='fpn_and_head')
            loss, class_loss, box_loss = self.loss_fn(class_out, box_out, s_cls, s_box, s_np)
            ood = None
            if s_roles is not None:
                ood_loss, ood_stats = self._ood_terms(class_out, s_cls, s_roles)
                loss = loss + ood_loss
                ood = dict(ood_stats, ood_loss=ood_loss.detach())
            vmf = None
            if self.vmf is not None:
                vmf_term, vmf = self._vmf_terms(s_cls)
                loss = loss + vmf_term
            loss.backward()
            # a GroupedOptimizer's step() records only its launches under capture: its step counts live on the device
            step_captured = opt.step if self._grouped else opt.step_captured
            norm = step_captured() if self.world == 1 else None
            outs = [loss.detach(), class_loss, box_loss, norm]
        g2 = None
        if self.world > 1:
            g2 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g2, pool=g1.pool()):
                outs[3] = step_captured()
        del feats, class_out, box_out, loss
        self._cap = (g1, g2, (sx, s_cls, s_box, s_np), outs)
        self._cap_ood = (s_roles, ood)
        self._cap_vmf = vmf

    def _replay(self, x, cls_t, box_t, npos, time_allreduce, roles=None):
        g1, g2, (sx, s_cls, s_box, s_np), outs = self._cap
        if tuple(x.shape) != tuple(sx.shape) or x.dtype != sx.dtype:
            raise ValueError('graph mode: input shape / dtype changed (%s %s, captured %s %s)' % (tuple(x.shape), x.dtype, tuple(sx.shape), sx.dtype))
        sx.copy_(x)
        base = self._static_base
        from .effdet.loss import _pack_targets
        # _pack_targets returns the common base only when the level tensors are the labeler's in-order views of it
        views = base is not None and cls_t[0]._base is not None and box_t[0]._base is not None
        cb = _pack_targets(list(cls_t), 0) if views else None
        bb = _pack_targets(list(box_t), 4) if views else None
        if base is not None and cb is not None and bb is not None and cb is cls_t[0]._base and bb is box_t[0]._base and \
                cb.shape == base[0].shape and bb.shape == base[1].shape:
            base[0].copy_(cb)
            base[1].copy_(bb)
        else:
            for d, t in zip(s_cls, cls_t):
                d.copy_(t)
            for d, t in zip(s_box, box_t):
                d.copy_(t)
        s_np.copy_(npos)
        if roles is not None:
            self._cap_ood[0].copy_(roles)
        if self._grouped:
            self.opt.refresh()                  # learning rates edited since the last replay reach the device tables
        else:
            self.opt.advance()
        g1.replay()
        if g2 is not None:
            self._allreduce(time_allreduce)
            g2.replay()
        self.model.invalidate()
        res = {'loss': outs[0].clone(), 'class_loss': outs[1].clone(), 'box_loss': outs[2].clone(),
               'grad_norm': None if outs[3] is None else outs[3].clone()}
        if roles is not None:
            res.update({k: v.clone() for k, v in self._cap_ood[1].items()})
        if self._cap_vmf is not None:
            res.update({k: v.clone() for k, v in self._cap_vmf.items()})
        self._synth_refresh()
        return res

    def _allreduce(self, time_allreduce):
        import torch.distributed as dist
        opt = self.opt
        if time_allreduce:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        dist.all_reduce(opt.flat_grad, op=dist.ReduceOp.SUM)
        opt.flat_grad.div_(self.world)
        if time_allreduce:
            e1.record()
            e1.synchronize()
            self.last_allreduce_ms = e0.elapsed_time(e1)

    def _engine_flags(self):
        eng = self.model._train_engine
        if eng is not None:
            eng.direct_grad = True          # FlatAdam owns every .grad (views of one flat buffer): add into them directly
            if self.synth is not None:
                eng.keep_penultimate = True
            if self.vmf is not None:
                eng.tower_output = True

    def __call__(self, x, target, time_allreduce=False, evaluator=None):
        model, opt = self.model, self.opt
        self._calls += 1
        if model._train_engine is None or model._train_engine.signature != model.train_signature():
            from .train_engine import TrainEngine
            model._train_engine = TrainEngine(model)
            if self._cap is not None:
                # The captured kernels hold raw addresses of the OLD engine's persistent tensors (folded weights, stage tables,
                # gradient buffers), which return to the allocator with it: replaying the graph would read freed memory.  Drop
                # the graph and its static buffers, run the eager warm-up again on the new engine, then re-capture.
                self._cap = None
                self._static_base = None
                self._calls = 1
        self._engine_flags()
        use_graph = self.graph and evaluator is None and self._calls > self._graph_warmup
        if self.synth is not None and self.graph:
            if not self.synth.fitted:
                # no fit (yet, or after a clear()): the step has no virtual side, so it runs eagerly, and a capture that holds one goes
                use_graph, self._cap, self._static_base, self._synth_eager = False, None, None, 0
            elif self._synth_eager < 1:
                use_graph = False               # the virtual side runs eagerly once before it is captured (its workspaces exist then)
        if use_graph:
            cls_t, box_t, npos = self.targets(target)
            roles = self.roles(target, cls_t)
            if self._cap is None:
                self._capture(x, cls_t, box_t, npos, roles)
            return self._replay(x, cls_t, box_t, npos, time_allreduce, roles)
        opt.zero_grad()
        cls_t, box_t, npos = self.targets(target)
        roles = self.roles(target, cls_t)
        feats = model(x, mode='bb')
        class_out, box_out = model(feats, mode='fpn_and_head')
        loss, class_loss, box_loss = self.loss_fn(class_out, box_out, cls_t, box_t, npos)
        ood = None
        if roles is not None:
            ood_loss, ood_stats = self._ood_terms(class_out, cls_t, roles)
            loss = loss + ood_loss
            ood = dict(ood_stats, ood_loss=ood_loss.detach())
            if self.synth is not None and self.synth.fitted:
                self._synth_eager += 1
        vmf = None
        if self.vmf is not None:
            vmf_term, vmf = self._vmf_terms(cls_t)
            loss = loss + vmf_term
        loss.backward()
        if evaluator is not None:
            self.evaluate(class_out, box_out, target, evaluator)
        if self.world > 1:
            self._allreduce(time_allreduce)
        norm = opt.step()
        model.invalidate()                      # the inference engine's packed weights are stale now
        res = {'loss': loss.detach(), 'class_loss': class_loss, 'box_loss': box_loss, 'grad_norm': norm}
        if ood is not None:
            res.update(ood)
        if vmf is not None:
            res.update(vmf)
        self._synth_refresh()
        return res
