"""The accurate mode (dtype 2, two-term bf16) at BiFPN widths above 160: tf_efficientdet_d4 (224) and d5 (288) run the fused
separable conv on an 8x8-pixel / 256-thread tile (csrc/sepconv.hip, dispatch_sep_pair_8x8), because the 8x16 tile's A tile no
longer fits in LDS there.  Kernel outputs against float64 arithmetic on the SAME representable inputs at 4e-5 of max|ref| (as in
test_accurate_gpu.py), whole networks against the float32 CPU oracle at north_star's 1e-3, and batch invariance at the bench
batches (the geometry follows from F alone)."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import model as om
from oracle import postprocess as op
from _sepconv_ref import sep_ref as _sep_ref      # float64 arithmetic of one fused node (R64)

DEV = 'cuda:0'
PAIR = 2
OUT_F32 = 4                   # dtype 6 = 2 | 4: two-term compute, float32 outputs
PAD_SYM = 1 << 24             # EFFDET_PAD_SYMMETRIC (pad_type ''): the on-the-fly 3x3 / s2 max pool pads 1 on both sides
TOLP = 4e-5


def _rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max() / (b.double().abs().max() + 1e-12))


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _enc(x):
    from ood_object_detection_amd import pairfmt
    return pairfmt.encode(x)


def _dec(t):
    from ood_object_detection_amd import pairfmt
    return pairfmt.decode(t.cpu())


def _q(x):
    """the value the two-term layout holds for x"""
    return _dec(_enc(x))


def _nhwc_q(x):
    """NCHW float -> (representable NCHW values, encoded NHWC device tensor)"""
    e = _enc(x.permute(0, 2, 3, 1).contiguous())
    return _dec(e).permute(0, 3, 1, 2).contiguous(), e.to(DEV)


# ------------------------------------------------------------------------------------------------------------------
# kernel level
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sym', [False, True])
@pytest.mark.parametrize('Fc', [160, 224, 288])
def test_sepconv_wide_bifpn_nodes_pair(Fc, sym):
    """three inputs (same size / nearest x2 / 3x3 s2 max pool of an odd-width map) fused as (x * w) / den, and two inputs
    (same size / max pool) fused as a plain weighted sum, in both max-pool pad conventions"""
    import _hip
    B, H, W = 2, 20, 12
    x_same, e_same = _nhwc_q(_rand(B, Fc, H, W, seed=20))
    x_up, e_up = _nhwc_q(_rand(B, Fc, H // 2, W // 2, seed=21))
    x_dn, e_dn = _nhwc_q(_rand(B, Fc, 2 * H, 2 * W - 1, seed=22))      # odd width: SAME pads one side only, '' both
    dw = _rand(Fc, 1, 3, 3, seed=23, scale=0.3)
    taps = dw.permute(2, 3, 0, 1).reshape(9, Fc).contiguous().to(DEV)
    pw = _q(_rand(Fc, Fc, seed=24, scale=Fc ** -0.5))
    wq = _enc(pw).to(DEV)
    scale, shift = torch.rand(Fc) + 0.5, _rand(Fc, seed=25, scale=0.1)
    sd, td = scale.to(DEV), shift.to(DEV)
    dt = PAIR | (PAD_SYM if sym else 0)
    pool_pad = '' if sym else 'same'
    desc = lambda ts, ms: [[(t.data_ptr(), t.shape[1] * t.shape[2] * t.shape[3], (t.shape[1], t.shape[2]), m) for t, m in zip(ts, ms)]]
    # three inputs
    fw, den = [0.7, 1.3, 0.4], 2.4001
    ref = _sep_ref([x_same, x_up, x_dn], [0, 1, 2], fw, den, 1, 1, dw, pw.reshape(Fc, Fc, 1, 1), None, scale, shift, 0, pool_pad)
    out = torch.empty(B, H, W, Fc, dtype=torch.float32, device=DEV)
    _hip.sepconv(dt, B, [(H, W)], desc([e_same, e_up, e_dn], (0, 1, 2)), 1, fw, den, 1, taps, wq, sd, td, [0], 0, Fc, Fc,
                 [out.data_ptr()], [H * W * Fc])
    torch.cuda.synchronize()
    err3 = _rel(_dec(out).permute(0, 3, 1, 2), ref)
    # two inputs
    fw2 = [0.9, 0.6]
    ref2 = _sep_ref([x_same, x_dn], [0, 2], fw2, 1.0, 2, 1, dw, pw.reshape(Fc, Fc, 1, 1), None, scale, shift, 0, pool_pad)
    out2 = torch.empty(B, H, W, Fc, dtype=torch.float32, device=DEV)
    _hip.sepconv(dt, B, [(H, W)], desc([e_same, e_dn], (0, 2)), 2, fw2, 1.0, 1, taps, wq, sd, td, [0], 0, Fc, Fc,
                 [out2.data_ptr()], [H * W * Fc])
    torch.cuda.synchronize()
    err2 = _rel(_dec(out2).permute(0, 3, 1, 2), ref2)
    assert err3 < TOLP and err2 < TOLP, (err3, err2)


@pytest.mark.parametrize('C', [90, 1, 64, 96])
@pytest.mark.parametrize('Fc', [160, 224, 288])
def test_sepconv_wide_head_levels_and_predicts_pair(Fc, C):
    """all five pyramid levels in one launch: a head layer (per-level affine, SiLU), the class predict (float32 logits + OOD energy
    / max-logit; at F = 288 the anchors' classes run as 64-row sub-chunks whose max / sum-exp carry over) and the box predict
    (36 float32 regressions)"""
    import _hip
    B, A = 2, 9
    hw = [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]
    offs = [0]
    for h, w in hw:
        offs.append(offs[-1] + h * w)
    P = offs[-1]
    fq, fe = zip(*[_nhwc_q(_rand(B, Fc, h, w, seed=30 + i)) for i, (h, w) in enumerate(hw)])
    pyr = torch.cat([e.reshape(B, -1, Fc) for e in fe], 1).contiguous()
    dw = _rand(Fc, 1, 3, 3, seed=36, scale=0.3)
    taps = dw.permute(2, 3, 0, 1).reshape(9, Fc).contiguous().to(DEV)
    es = 4
    li = [[(pyr.data_ptr() + offs[l] * Fc * es, P * Fc, hw[l], 0)] for l in range(5)]
    # head layer
    pw = _q(_rand(Fc, Fc, seed=37, scale=Fc ** -0.5))
    scale, shift = torch.rand(5, Fc) + 0.5, _rand(5, Fc, seed=38, scale=0.1)
    out = torch.empty(B, P, Fc, dtype=torch.float32, device=DEV)
    wq, sd, td = _enc(pw).to(DEV), scale.to(DEV), shift.to(DEV)
    _hip.sepconv(PAIR, B, hw, li, 0, [], 1.0, 0, taps, wq, sd, td, list(range(5)), 1, Fc, Fc,
                 [out.data_ptr() + offs[l] * Fc * es for l in range(5)], [P * Fc] * 5)
    torch.cuda.synchronize()
    got_all = _dec(out)
    for l in range(5):
        ref = _sep_ref([fq[l]], [0], [], 1.0, 0, 0, dw, pw.reshape(Fc, Fc, 1, 1), None, scale[l], shift[l], 1)
        got = got_all[:, offs[l]:offs[l + 1], :].reshape(B, hw[l][0], hw[l][1], Fc).permute(0, 3, 1, 2)
        assert _rel(got, ref) < TOLP, ('head layer', l)
    # class predict + OOD
    NO = A * C
    pwp = _q(_rand(NO, Fc, seed=39, scale=2.0 * Fc ** -0.5))
    bias = _rand(NO, seed=40, scale=0.5) - 2.0
    N = A * P
    cls_all = torch.full((B, N, C), float('nan'), dtype=torch.float32, device=DEV)
    energy = torch.empty(B, N, dtype=torch.float32, device=DEV)
    maxl = torch.empty(B, N, dtype=torch.float32, device=DEV)
    wpq, bd = _enc(pwp).to(DEV), bias.reshape(1, NO).to(DEV)
    _hip.sepconv(PAIR | OUT_F32, B, hw, li, 0, [], 1.0, 0, taps, wpq, None, bd,
                 [0] * 5, 0, Fc, NO, [cls_all.data_ptr() + offs[l] * NO * es for l in range(5)], [P * NO] * 5,
                 ood=dict(classes=C, energy=energy, maxlogit=maxl, stride=N, level_off=[o * A for o in offs[:5]]), A=A)
    torch.cuda.synchronize()
    refs = [_sep_ref([fq[l]], [0], [], 1.0, 0, 0, dw, pwp.reshape(NO, Fc, 1, 1), bias, None, torch.zeros(NO), 0) for l in range(5)]
    ref_all = torch.cat([r.permute(0, 2, 3, 1).reshape(B, -1, C) for r in refs], 1)
    assert _rel(cls_all, ref_all) < TOLP
    e_ref = -torch.logsumexp(ref_all, dim=2)
    m_ref = ref_all.max(dim=2).values
    assert float((energy.cpu().double() - e_ref).abs().max()) < 1e-4 * max(1.0, float(e_ref.abs().max()))
    assert float((maxl.cpu().double() - m_ref).abs().max()) < 1e-4 * max(1.0, float(m_ref.abs().max()))
    # box predict
    NB = A * 4
    pwb = _q(_rand(NB, Fc, seed=41, scale=Fc ** -0.5))
    biasb = _rand(NB, seed=42, scale=0.1)
    box_all = torch.full((B, P, NB), float('nan'), dtype=torch.float32, device=DEV)
    wbq, bbd = _enc(pwb).to(DEV), biasb.reshape(1, NB).to(DEV)
    _hip.sepconv(PAIR | OUT_F32, B, hw, li, 0, [], 1.0, 0, taps, wbq, None, bbd, [0] * 5, 0, Fc, NB,
                 [box_all.data_ptr() + offs[l] * NB * es for l in range(5)], [P * NB] * 5)
    torch.cuda.synchronize()
    refs = [_sep_ref([fq[l]], [0], [], 1.0, 0, 0, dw, pwb.reshape(NB, Fc, 1, 1), biasb, None, torch.zeros(NB), 0) for l in range(5)]
    ref_all = torch.cat([r.permute(0, 2, 3, 1).reshape(B, -1, NB) for r in refs], 1)
    assert _rel(box_all, ref_all) < TOLP


# ------------------------------------------------------------------------------------------------------------------
# whole networks against the float32 CPU oracle
# ------------------------------------------------------------------------------------------------------------------
def _linf(a, b):
    return float((a.float().cpu() - b.float().cpu()).abs().max())


@pytest.mark.parametrize('name,size', [('tf_efficientdet_d3', 256), ('tf_efficientdet_d4', 384), ('tf_efficientdet_d5', 384)])
def test_accurate_mode_wide_bifpn_matches_the_oracle(name, size):
    """class logits, box regressions and OOD scores against the oracle within 3e-4 of max|logit| (measured 1.1e-4 / 1.6e-4 /
    1.05e-4 for d3 / d4 / d5; these seeded small-image networks reach |logit| 3.7 / 8.0 / 5.0, so d4 is 1.3e-3 in absolute terms -
    the 1e-3 north-star check at BASELINE config 4's real size is test_accurate_mode_d4_1024_soft_nms); image 0 alone gives the
    same bits as in the batch; 'bb' features against the oracle's backbone, and 'fpn_and_head' on them reproduces the full forward"""
    from _models import seeded_model
    from _seeded import seeded_array
    C = 20
    model, cfg, nodes, sd = seeded_model(name, size, C, seed=15, cls_bias=-2.0)
    x = torch.from_numpy(seeded_array(16, 'input', (2, 3, size, size)))
    with torch.no_grad():
        cls_r, box_r = om.efficientdet_forward(sd, cfg, x, nodes)
        e_ref, m_ref = om.ood_scores(cls_r, C)
        fr = om.backbone_forward(sd, cfg.backbone_name, x, pad_type=cfg.pad_type)
    model = model.to(DEV).float()
    model.compute_mode = 'accurate'
    xd = x.to(DEV)
    with torch.no_grad():
        cls_o, box_o = model(xd)
        cls_o, box_o = [t.clone() for t in cls_o], [t.clone() for t in box_o]
        e2, m2 = model.ood_energy.clone(), model.ood_max_logit.clone()
    assert model._engine.dt == PAIR
    err = dict(cls=max(_linf(a, r) for a, r in zip(cls_o, cls_r)), box=max(_linf(a, r) for a, r in zip(box_o, box_r)),
               energy=_linf(e2, e_ref), max_logit=_linf(m2, m_ref))
    zmax = max(float(r.abs().max()) for r in cls_r)
    print('%s %d px accurate vs oracle (max|logit| %.2f):' % (name, size, zmax), err)
    assert max(err.values()) <= 3e-4 * max(1.0, zmax), err
    with torch.no_grad():
        cls1, box1 = model(xd[:1])
        for a, r in zip(list(cls1) + list(box1), cls_o + box_o):
            assert torch.equal(a[0], r[0]), 'image 0 differs between B = 1 and B = 2'
        assert torch.equal(model.ood_energy[0], e2[0]) and torch.equal(model.ood_max_logit[0], m2[0])
        feats = model(xd, mode='bb')
        for a, b in zip(feats, fr):
            assert _linf(a, b) <= 1e-3 * max(1.0, float(b.abs().max()))
        cls3, box3 = model([f.contiguous() for f in feats], mode='fpn_and_head')
    reentry = max(_linf(a, b) for a, b in zip(list(cls3) + list(box3), cls_o + box_o))
    print('%s: fpn_and_head on the decoded features vs the full forward %.2e' % (name, reentry))
    assert reentry <= 2e-4 * max(1.0, zmax)


def _decode(rel, a):
    ya, xa, ha, wa = (a[:, 0] + a[:, 2]) / 2, (a[:, 1] + a[:, 3]) / 2, a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
    w, h = torch.exp(rel[:, 3]) * wa, torch.exp(rel[:, 2]) * ha
    yc, xc = rel[:, 0] * ha + ya, rel[:, 1] * wa + xa
    return torch.stack([xc - w / 2, yc - h / 2, xc + w / 2, yc + h / 2], 1)


def test_accurate_mode_d4_1024_soft_nms():
    """BASELINE config 4 at its real size in the accurate mode, one image: (i) head outputs and OOD scores within 1e-3 of the
    oracle, (ii) post-processing at 196 416 anchors against the oracle fed the SAME logits (classes exact, scores 1e-5, boxes
    2e-4 px: measured 6.1e-5), the kept detections' boxes against the oracle's regressions decoded at the same anchors (5e-3 px:
    measured 1.6e-3; head outputs measured 4.9e-5), and (iii) one hipGraph capture of DetBenchPredict replays the eager
    detections bit for bit."""
    from _models import seeded_model
    from _seeded import seeded_array
    from ood_object_detection_amd.effdet.bench import DetBenchPredict
    name, size, ncls = 'tf_efficientdet_d4', 1024, 90
    model, cfg, nodes, sd = seeded_model(name, size, ncls, seed=21, cls_bias=-2.0, soft_nms=True)
    x = torch.from_numpy(seeded_array(21, 'input', (1, 3, size, size)))
    with torch.no_grad():
        cls_r, box_r = om.efficientdet_forward(sd, cfg, x, nodes)
    m = copy.deepcopy(model).to(DEV).float()
    m.compute_mode = 'accurate'
    bench = DetBenchPredict(m, streams=1).to(DEV)
    xd = x.to(DEV)
    with torch.no_grad():
        det = bench(xd).clone()
    torch.cuda.synchronize()
    eng = m._engine
    assert eng.dt == PAIR
    cls_g = [t.float().cpu() for t in eng.head_views(eng.cls_all, ncls)]
    box_g = [t.float().cpu() for t in eng.head_views(eng.box_all, 4)]
    # (i)
    err_c = max(_linf(a, r) for a, r in zip(cls_g, cls_r))
    err_b = max(_linf(a, r) for a, r in zip(box_g, box_r))
    e_ref, m_ref = om.ood_scores(cls_r, ncls)
    err_e, err_m = _linf(m.ood_energy, e_ref), _linf(m.ood_max_logit, m_ref)
    # (ii)
    anchors = op.anchor_boxes(cfg.min_level, cfg.max_level, cfg.num_scales, cfg.aspect_ratios, cfg.anchor_scale, (size, size))
    assert anchors.shape[0] == 196416
    c, b, idx, cl = op.post_process(cls_g, box_g, 5, ncls, 5000)
    ref, src = op.generate_detections(c[0], b[0], anchors, idx[0], cl[0], None, torch.tensor(size), 100, True, return_aux=True)
    n = int(bench.last_count[0])
    assert n == ref.shape[0] and n > 0
    got = det[0, :n].float().cpu()
    assert torch.equal(got[:, 5], ref[:, 5])
    err_s = float((got[:, 4] - ref[:, 4]).abs().max())
    box_same = float((got[:, :4] - ref[:, :4]).abs().max())
    e_same, _ = om.ood_scores(cls_g, ncls)
    a_idx = idx[0][src]
    err_es = float((bench.last_ood['energy'][0, :n].cpu() - e_same[0][a_idx]).abs().max())
    box_ref_all = torch.cat([r.permute(0, 2, 3, 1).reshape(1, -1, 4) for r in box_r], 1)[0]
    kept = bench.last_ood['anchor_index'][0, :n].cpu().long()
    box_oracle = float((_decode(box_ref_all[kept], anchors.float()[kept]) - got[:, :4]).abs().max())
    print('d4 1024 accurate: logits %.2e regressions %.2e energy %.2e max-logit %.2e | %d detections: scores %.2e, boxes %.2e px '
          '(same logits), %.2e px (oracle regressions), energy %.2e' % (err_c, err_b, err_e, err_m, n, err_s, box_same, box_oracle, err_es))
    assert err_c <= 1e-3 and err_b <= 1e-3 and err_e <= 1e-3 and err_m <= 1e-3
    assert err_s <= 1e-5 and err_es <= 1e-4
    assert box_same <= 2e-4 and box_oracle <= 5e-3
    # (iii)
    with torch.no_grad():
        side = torch.cuda.Stream(DEV)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            out = bench(xd)
        g.replay()
        torch.cuda.synchronize()
    assert torch.equal(out, det)


# ------------------------------------------------------------------------------------------------------------------
# batch invariance at the bench batches
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,size,batch,images', [('tf_efficientdet_d0', 640, 64, (0, 37, 63)),
                                                    ('tf_efficientdet_d4', 1024, 8, (0, 7))])
def test_accurate_mode_batch_invariance(name, size, batch, images):
    """image i of the bench batch is bit-equal to the same image run alone (class / box outputs and OOD scores)"""
    import bench as B
    model = B.build_model(name, size, 90).to(DEV).float()
    model.compute_mode = 'accurate'
    x = torch.randn(batch, 3, size, size, device=DEV, generator=torch.Generator(device=DEV).manual_seed(7))
    with torch.no_grad():
        cb, bb = model(x)
        cb, bb = [t.clone() for t in cb], [t.clone() for t in bb]
        eb, mb = model.ood_energy.clone(), model.ood_max_logit.clone()
        assert model._engine.dt == PAIR
        for i in images:
            c1, b1 = model(x[i:i + 1])
            for a, r in zip(list(c1) + list(b1), cb + bb):
                assert torch.equal(a[0], r[i]), 'image %d differs between B = 1 and B = %d' % (i, batch)
            assert torch.equal(model.ood_energy[0], eb[i]) and torch.equal(model.ood_max_logit[0], mb[i])
