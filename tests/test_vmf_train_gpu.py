"""The vMF head in the network: the gradient path from the class tower (TrainEngine.tower_output), PretrainStep(vmf_head=...) and
DetBenchPredict with VMFFeatureOOD, on tf_efficientdet_d0 at 128 px with two images - the size of __graft_entry__.smoke, whose CPU
replica (torch autograd through the oracle, BatchNorm on running statistics) and bound are used: every gradient tensor within 2e-3
of its own largest entry, with a floor of 1e-4 of the largest gradient entry of all."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SIZE, PB, PC = 128, 2, 20


def _train_setup():
    from _models import seeded_model
    from _seeded import seeded_array
    model, cfg, nodes, sd = seeded_model('tf_efficientdet_d0', SIZE, PC, seed=11)
    x = torch.from_numpy(seeded_array(11, 'input', (PB, 3, SIZE, SIZE)))
    rs = np.random.RandomState(5)
    cls_t, box_t = [], []
    for l in range(cfg.num_levels):
        s = SIZE // (2 ** (cfg.min_level + l))
        cls_t.append(torch.from_numpy(rs.choice([-2, -1, -1, -1, -1, 0, 3, PC - 1], size=(PB, s, s, 9)).astype(np.int64)))
        t = rs.normal(0, 0.2, (PB, s, s, 36)).astype(np.float32)
        t[rs.uniform(size=t.shape) < 0.7] = 0.0
        box_t.append(torch.from_numpy(t))
    return model, cfg, nodes, sd, x, cls_t, box_t, torch.tensor([7.0, 4.0])


def _oracle_tower(om, sdg, cfg, x, nodes):
    """-> (class outputs, box outputs, the class tower per level [B, F, h, w]) through the oracle's own pieces"""
    info = om.backbone_feature_info(cfg.backbone_name)
    feats = om.backbone_forward(sdg, cfg.backbone_name, x, pad_type=cfg.pad_type)
    activs = om.bifpn_forward(sdg, cfg, feats, nodes, info)
    eps = cfg.norm_kwargs['eps']
    tower = []
    for level in range(cfg.num_levels):
        t = activs[level]
        for r in range(cfg.box_class_repeats):
            t = om._sepconv(t, sdg, 'class_net.conv_rep.%d.' % r, cfg.pad_type)
            t = om.silu(om.bn_eval(t, sdg, 'class_net.bn_rep.%d.%d.bn.' % (r, level), eps))
        tower.append(t)
    return om.head_forward(sdg, cfg, activs, 'class_net.'), om.head_forward(sdg, cfg, activs, 'box_net.'), tower


def _device_run(model, sd, cfg, x, cls_t, box_t, npos, flag, weights, det=True):
    """one forward + backward on the device -> (outputs, {name: grad}); weights: per-level [B, F, h, w] for sum(tower * w), or None"""
    from ood_object_detection_amd.effdet.loss import DetectionLoss
    from ood_object_detection_amd.train_engine import TrainEngine
    model.load_state_dict(sd)
    model.train()
    model.apply(lambda m: m.eval() if isinstance(m, torch.nn.BatchNorm2d) else None)
    model.zero_grad(set_to_none=True)
    eng = model._train_engine = TrainEngine(model)
    eng.tower_output = flag
    cls_o, box_o = model(model(x.to(DEV), mode='bb'), mode='fpn_and_head')
    total = None
    if det:
        total, _, _ = DetectionLoss(cfg)(cls_o, box_o, [t.to(DEV) for t in cls_t], [t.to(DEV) for t in box_t], npos.to(DEV))
    if weights is not None:
        assert eng.class_tower is not None and all(t.requires_grad for t in eng.class_tower)
        extra = sum((t * w.to(DEV)).sum() for t, w in zip(eng.class_tower, weights))
        total = extra if total is None else total + extra
    else:
        assert (eng.class_tower is not None) == flag
    total.backward()
    torch.cuda.synchronize()
    outs = [t.detach().clone() for t in list(cls_o) + list(box_o)]
    tower = None if eng.class_tower is None else [t.detach().float().cpu() for t in eng.class_tower]
    return outs, {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in model.named_parameters()}, total.detach(), tower


def _compare(grads, ref, what):
    gmax = max(float(g.abs().max()) for g in ref.values() if g is not None)
    worst, n = 0.0, 0
    for name, r in ref.items():
        if r is None or name.endswith('edge_weights'):
            continue
        assert grads.get(name) is not None, (what, name)
        worst = max(worst, float((grads[name].cpu() - r).abs().max()) / max(float(r.abs().max()), 1e-4 * gmax))
        n += 1
    print('%s: %d tensors, largest gradient entry %.3e, worst relative error %.2e (bound 2e-3)' % (what, n, gmax, worst))
    assert n > 0 and worst <= 2e-3, (what, worst)
    return n


def test_tower_gradient_reaches_the_tower_and_the_bifpn():
    from oracle import model as om
    from oracle import train as ot
    model, cfg, nodes, sd, x, cls_t, box_t, npos = _train_setup()
    cfg.alpha, cfg.box_loss_weight = 0.15, 50.0
    model = model.to(DEV).float()
    g = torch.Generator().manual_seed(7)
    sdg = {k: (v.clone().float().requires_grad_() if v.is_floating_point() and 'running' not in k else v.clone()) for k, v in sd.items()}
    cls_r, box_r, tower_r = _oracle_tower(om, sdg, cfg, x, nodes)
    weights = [torch.randn(t.shape, generator=g) for t in tower_r]
    det_r, _, _ = ot.detection_loss(cls_r, box_r, cls_t, box_t, npos, PC, 0.15, 0.1, 50.0)
    tow_r = sum((t * w).sum() for t, w in zip(tower_r, weights))
    names = [k for k, v in sdg.items() if torch.is_tensor(v) and v.requires_grad]
    ref_tow = dict(zip(names, torch.autograd.grad(tow_r, [sdg[k] for k in names], allow_unused=True, retain_graph=True)))
    ref_both = dict(zip(names, torch.autograd.grad(det_r + tow_r, [sdg[k] for k in names], allow_unused=True)))
    # flag off, and flag on with the tower not read by the loss: the same outputs and gradients bit for bit
    o_off, g_off, t_off, _ = _device_run(model, sd, cfg, x, cls_t, box_t, npos, False, None)
    o_on, g_on, t_on, tower = _device_run(model, sd, cfg, x, cls_t, box_t, npos, True, None)
    assert torch.equal(t_off, t_on) and all(torch.equal(a, b) for a, b in zip(o_off, o_on))
    assert set(g_off) == set(g_on)
    for n in g_off:
        assert (g_off[n] is None) == (g_on[n] is None) and (g_off[n] is None or torch.equal(g_off[n], g_on[n])), n
    for t, r in zip(tower, tower_r):
        assert float((t - r.detach()).abs().max()) <= 1e-3 * max(1.0, float(r.abs().max()))
    # the tower gradient alone: no gradient arrives for the class or the box outputs
    _, g_tow, _, _ = _device_run(model, sd, cfg, x, cls_t, box_t, npos, True, weights, det=False)
    n = _compare(g_tow, ref_tow, 'tower loss alone')
    live = [k for k, v in ref_tow.items() if v is not None and not k.endswith('edge_weights')]
    assert n == len(live) and any(k.startswith('fpn.') for k in live) and any(k.startswith('class_net.conv_rep') for k in live)
    assert any(k.startswith('backbone.') for k in live)
    assert all(g_tow[k] is None for k in g_tow if k.startswith('box_net.') or k.startswith('class_net.predict.'))
    # together with the detection loss
    _, g_both, total, _ = _device_run(model, sd, cfg, x, cls_t, box_t, npos, True, weights)
    assert abs(float(total) - float(det_r + tow_r)) <= 1e-4 * abs(float(det_r + tow_r))
    _compare(g_both, ref_both, 'detection loss + tower loss')
    model.eval()


# ---- PretrainStep ---------------------------------------------------------------------------------------------------------------
def _pretrain_inputs(steps):
    g = torch.Generator().manual_seed(3)
    xs = [torch.randint(0, 256, (PB, 3, SIZE, SIZE), generator=g, dtype=torch.uint8).to(DEV) for _ in range(steps)]
    boxes = [torch.tensor([[10., 12., 70., 90.], [40., 30., 120., 100.]]), torch.tensor([[5., 5., 60., 50.]])]
    cls = [torch.tensor([3, 7]), torch.tensor([1])]
    return xs, {'bbox': [b.to(DEV) for b in boxes], 'cls': [c.to(DEV) for c in cls]}


def _model():
    from _models import seeded_model
    model, cfg, _, _ = seeded_model('tf_efficientdet_d0', SIZE, PC, seed=23)
    return model.to(DEV).float()


def _vmf(model, dim=16):
    from ood_object_detection_amd.ood_vmf import VMFHead
    A = model.class_net.predict.conv_pw.weight.shape[0] // PC
    return VMFHead(model.config.fpn_channels, PC, A, dim=dim).to(DEV)


def _state(*modules):
    out = {}
    for i, m in enumerate(modules):
        out.update({'%d.%s' % (i, n): t.detach().clone() for n, t in list(m.named_parameters()) + list(m.named_buffers())})
    return out


def test_pretrain_step_with_the_vmf_head_eager_and_graph():
    from ood_object_detection_amd.pretrain import PretrainStep
    xs, target = _pretrain_inputs(4)
    runs = []
    for graph in (False, True):
        model = _model()
        head = _vmf(model)
        before = _state(head)
        step = PretrainStep(model, vmf_head=head, vmf_weight=1.5, graph=graph, graph_warmup=2)
        hist = []
        for x in xs:
            o = step(x, target)
            assert float(o['vmf_loss']) > 0.0 and int(o['vmf_m']) > 0 and int(o['vmf_skipped']) == 0
            hist.append((o['loss'].item(), o['vmf_loss'].item(), o['grad_norm'].item(), int(o['vmf_m']), int(o['vmf_valid_classes'])))
        if graph:
            assert step._cap is not None
        after = _state(head)
        for n in ('0.weight1', '0.weight2', '0.log_kappa'):
            assert not torch.equal(before[n], after[n]), n                       # the head's parameters are in the optimizer
        # the classes the labels name have prototypes: unit vectors; the others stay zero
        assert int(head.valid.sum()) == hist[-1][4] >= 1
        norms = head.prototypes[head.valid.bool()].norm(dim=1)
        assert float((norms - 1).abs().max()) <= 1e-5 and not head.prototypes[~head.valid.bool()].any()
        runs.append((hist, _state(model, head)))
    assert runs[0][0] == runs[1][0], (runs[0][0], runs[1][0])
    for n in runs[0][1]:
        assert torch.equal(runs[0][1][n], runs[1][1][n]), n


def test_pretrain_step_loss_is_the_detection_loss_plus_the_weighted_vmf_loss():
    from ood_object_detection_amd.pretrain import PretrainStep
    xs, target = _pretrain_inputs(1)
    plain_model = _model()
    plain = PretrainStep(plain_model)(xs[0], target)
    assert 'vmf_loss' not in plain and plain_model._train_engine.tower_output is False and plain_model._train_engine.class_tower is None
    model = _model()
    o = PretrainStep(model, vmf_head=_vmf(model), vmf_weight=1.5)(xs[0], target)
    assert torch.equal(o['class_loss'], plain['class_loss']) and torch.equal(o['box_loss'], plain['box_loss'])
    assert torch.equal(o['loss'], plain['loss'] + 1.5 * o['vmf_loss']) and float(o['grad_norm']) != float(plain['grad_norm'])
    with pytest.raises(ValueError, match='vmf_head'):
        from ood_object_detection_amd.ood_vmf import VMFHead
        PretrainStep(_model(), vmf_head=VMFHead(64, PC + 1, 9))


# ---- DetBenchPredict ---------------------------------------------------------------------------------------------------------------
def test_det_bench_predict_carries_the_vmf_keys():
    from _models import seeded_model
    from _seeded import seeded_array
    from ood_object_detection_amd import ood
    from ood_object_detection_amd.effdet.bench import DetBenchPredict
    from ood_object_detection_amd.ood_features import KNNFeatureOOD
    from ood_object_detection_amd.ood_vmf import VMFFeatureOOD, VMFHead
    model, cfg, _, _ = seeded_model('tf_efficientdet_d0', 128, 3, seed=21, cls_bias=-2.0)
    model = copy.deepcopy(model).to(DEV).float()
    x = torch.from_numpy(seeded_array(22, 'input', (4, 3, 128, 128))).to(DEV)
    plain = DetBenchPredict(model, streams=1).to(DEV)
    det0 = plain(x).clone()
    cnt0, ood0 = plain.last_count.clone(), {k: v.clone() for k, v in plain.last_ood.items()}
    n_det = int(cnt0.sum())
    assert n_det > 0
    A, F = plain.anchors.get_anchors_per_location(), cfg.fpn_channels
    head = VMFHead(F, 3, A, dim=64).to(DEV)
    scorer = VMFFeatureOOD(head)
    bench = DetBenchPredict(model, streams=1, feature_ood=[scorer]).to(DEV)
    assert model.keep_class_tower is True
    model(x)
    tower = model._engine.class_tower_views()
    P = sum(t.shape[2] * t.shape[3] for t in tower)
    labels = torch.randint(-2, 3, (4, A * P), generator=torch.Generator().manual_seed(4)).to(DEV)
    with torch.no_grad():
        _, stats = head(tower, labels)                           # prototypes from the tower itself
    assert int(stats['m']) > 0 and bool(head.valid.all())
    det1 = bench(x)
    torch.cuda.synchronize()
    assert torch.equal(det1, det0) and torch.equal(bench.last_count, cnt0)
    assert set(bench.last_ood) == set(ood0) | set(scorer.KEYS)
    for k in ood0:
        assert torch.equal(bench.last_ood[k], ood0[k]), k
    got = {k: bench.last_ood[k].clone() for k in scorer.KEYS}
    direct = scorer.score(model._engine.class_tower_views(), ood0['anchor_index'], cnt0)
    for k in scorer.KEYS:
        assert torch.equal(got[k], direct[k]), k
    live = torch.arange(det0.shape[1], device=DEV)[None] < cnt0[:, None]
    assert got['vmf'].dtype == torch.float32 and got['vmf_class'].dtype == torch.int64 and tuple(got['vmf'].shape) == tuple(det0.shape[:2])
    assert bool(((got['vmf_class'][live] >= 0) & (got['vmf_class'][live] < 3)).all()) and bool(torch.isfinite(got['vmf'][live]).all())
    assert bool((got['vmf_class'][~live] == -1).all()) and not got['vmf'][~live].any() and not got['vmf_cosine'][~live].any()
    assert float(got['vmf_cosine'][live].abs().max()) <= 1.0 + 1e-5
    two = DetBenchPredict(model, streams=2, feature_ood=[scorer]).to(DEV)
    two(x)
    torch.cuda.synchronize()
    for k in scorer.KEYS:
        assert torch.equal(two.last_ood[k], got[k]), k
    # a score feeds the evaluator without a conversion
    ev = ood.OODEvaluator(4 * bench.max_det_per_image, 4 * bench.max_det_per_image, DEV)
    ev.add_detections(got['vmf'], cnt0, False)
    ev.add_detections(got['vmf'] - 1.0, cnt0, True)
    res = ev.evaluate()
    assert res['n_in'] == res['n_ood'] == n_det
    # SIREN's k-NN variant: at dim = 64 the unit embeddings are a feature tensor of KNNFeatureOOD
    emb = scorer.embeddings(tower)
    knn = KNNFeatureOOD(64, A, capacity=4 * P * A, k=3)
    knn.add(emb)
    knn.fit()
    out = knn.score(emb, ood0['anchor_index'], cnt0)
    assert tuple(out['knn'].shape) == tuple(det0.shape[:2]) and bool(torch.isfinite(out['knn'][live]).all())
