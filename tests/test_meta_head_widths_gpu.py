"""MetaHead's no-grad forward (the META form of sepconv_kernel + bn_batch_stats_kernel) and its differentiable path at every
BiFPN width, against the float64 oracle, on maps that are non-square, span several tiles and end in partial tiles for both
the 8 x 8 float32 and the 8 x 16 bf16 tiling; batch statistics over 4 and 2 samples; and the batch statistics of one layer in
isolation on channels whose mean is many standard deviations from zero.  The inputs, their seeds and the bound of the
statistics test are fixed and justified on the CPU by tests/test_meta_head_widths_host.py (cases: tests/_meta_head_cases.py).

Every test prints the figures it asserts on."""
import copy
import functools

import pytest
import torch

import _meta_head_cases as mc
from oracle import model as om

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
WIDTH_IDS = [str(f) for _, f, _ in mc.WIDTHS]
DTYPES = [torch.float32, torch.bfloat16]
DT_IDS = ['f32', 'bf16']


@functools.lru_cache(maxsize=None)
def _head(f, seed, sep_head=False):
    return mc.build_meta_head(mc.NAME_OF[f], seed, sep_head=sep_head)


def _module(f, seed, dtype, sep_head=False):
    cfg, _, _, mh = _head(f, seed, sep_head)
    return cfg, copy.deepcopy(mh).to(DEV).to(dtype)


def _reference(mh, xr, **kw):
    """float64 oracle on the values the module holds (bf16: the rounded weights and inputs)"""
    P = lambda ps: [p.detach().double().cpu() for p in ps]
    with torch.no_grad():
        return om.meta_head_forward(P(mh.conv_dw_rep), P(mh.conv_pw_rep), P(mh.conv_pb_rep), P(mh.bn_rep_w), P(mh.bn_rep_b), P(mh.predict),
                                    [t.double().cpu() for t in xr], dtype=torch.float64, **kw)


@functools.lru_cache(maxsize=None)
def _forward_case(f, dtype, kind):
    """module, device inputs, GPU result and float64 reference of one (width, dtype, level list): computed once, read by several tests"""
    seed, levels = (mc.MAIN_SEED[f], mc.MAIN_LEVELS) if kind == 'main' else mc.FEW_CASE[f]
    cfg, mh = _module(f, seed, dtype)
    x = [t.to(DEV).to(dtype) for t in mc.level_inputs(seed, f, levels)]
    with torch.no_grad():
        outs, activs = mh(x, ret_activs=True)
    torch.cuda.synchronize()
    ro, ra = _reference(mh, x)
    return dict(cfg=cfg, mh=mh, x=x, levels=levels, outs=outs, activs=activs, ro=ro, ra=ra)


def _check(tag, got, ref, dtype):
    """the project's bounds (tests/test_model_gpu.py::test_meta_head_forward): float32 max|a - b| <= 2e-4 max(1, |b|max), bf16
    relative rms <= 0.05.  Prints every figure, then asserts on all of them."""
    assert len(got) == len(ref)
    bad = []
    for i, (a, b) in enumerate(zip(got, ref)):
        assert tuple(a.shape) == tuple(b.shape) and a.dtype == dtype
        assert bool(torch.isfinite(a.float()).all())
        e, bound = (mc.f32_error(a, b), mc.F32_BOUND) if dtype == torch.float32 else (mc.rel_rms(a, b), mc.BF16_RMS_BOUND)
        print('%s[%d] %s: %.3e (bound %.1e)' % (tag, i, tuple(b.shape[2:]), e, bound))
        if not e <= bound:
            bad.append((tag, i, e))
    assert not bad, bad


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('name,f,r', mc.WIDTHS, ids=WIDTH_IDS)
def test_forward_every_width(name, f, r, dtype):
    c = _forward_case(f, dtype, 'main')
    assert c['cfg'].box_class_repeats == r and c['mh'].num_layers == r and c['mh'].num_channels == f
    for o, a, (h, w) in zip(c['outs'], c['activs'], mc.MAIN_LEVELS):
        assert tuple(o.shape) == (mc.B, 9, h, w) and tuple(a.shape) == (mc.B, f, h, w)
    _check('F%d outputs' % f, c['outs'], c['ro'], dtype)
    _check('F%d activations' % f, c['activs'], c['ra'], dtype)


@pytest.mark.parametrize('name,f,r', mc.WIDTHS, ids=WIDTH_IDS)
def test_few_sample_levels(name, f, r):
    """batch statistics over 16, 4 and 2 samples per channel: the variance is a small difference of the layer's outputs"""
    c = _forward_case(f, torch.float32, 'few')
    print('F%d seed %d levels %s' % (f, mc.FEW_CASE[f][0], c['levels']))
    _check('F%d outputs' % f, c['outs'], c['ro'], torch.float32)
    _check('F%d activations' % f, c['activs'], c['ra'], torch.float32)


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('f', [88, 224])
def test_packed_input_views(f, dtype):
    """the levels as NCHW views of one packed [B, P, F] buffer (image stride P * F, as the engine's pyramid hands them over):
    taken as they are, bit-equal to the contiguous call"""
    c = _forward_case(f, dtype, 'main')
    P = sum(h * w for h, w in mc.MAIN_LEVELS)
    buf = torch.empty(mc.B, P, f, dtype=dtype, device=DEV)
    views, off = [], 0
    for t, (h, w) in zip(c['x'], mc.MAIN_LEVELS):
        buf[:, off:off + h * w] = t.permute(0, 2, 3, 1).reshape(mc.B, h * w, f)
        views.append(buf[:, off:off + h * w].view(mc.B, h, w, f).permute(0, 3, 1, 2))
        off += h * w
    assert all(v.stride(0) == P * f and torch.equal(v, t) for v, t in zip(views, c['x']))
    with torch.no_grad():
        outs, activs = c['mh'](views, ret_activs=True)
    for a, b in zip(outs + activs, c['outs'] + c['activs']):
        assert torch.equal(a, b)


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('f', [88, 288])
def test_other_head_forms(f, dtype):
    c = _forward_case(f, dtype, 'main')
    mh, x = c['mh'], c['x']
    with torch.no_grad():
        fw = mh.conv_dw_rep + mh.conv_pw_rep + mh.conv_pb_rep + mh.predict + mh.bn_rep_w + mh.bn_rep_b
        outs2 = mh(x, fast_weights=fw)
        assert len(outs2) == len(c['outs']) and all(torch.equal(a, b) for a, b in zip(outs2, c['outs']))
        outs3 = mh(x, level_offset=2)
        assert len(outs3) == 3 and all(torch.equal(a, b) for a, b in zip(outs3, c['outs'][2:]))
        # separate class head on the same x_pred
        _, mhs = _module(f, mc.MAIN_SEED[f], dtype, sep_head=True)
        co, ao, act = mhs(x, ret_activs=True, heads='both')
        rco = _reference(mhs, x, predict_class=[p.detach().double().cpu() for p in mhs.predict_class])[2]
    _check('F%d class head' % f, co, rco, dtype)
    assert all(torch.equal(a, b) for a, b in zip(ao, c['outs'])) and all(torch.equal(a, b) for a, b in zip(act, c['activs']))


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
def test_too_wide_is_refused_cleanly(dtype):
    """384 channels: the A tile and a 64-row W chunk pass the 160 KiB of LDS in both dtypes; the first layer's call returns
    EFFDET_EINVAL before anything is launched, and the next valid call is unaffected"""
    from ood_object_detection_amd.effdet.meta_head import MetaHead
    cfg, init, extra = mc.head_weights('tf_efficientdet_d0', 3, fpn_channels=384)
    assert cfg.fpn_channels == 384 and mc.config_of('tf_efficientdet_d0').fpn_channels == 64
    mh = MetaHead(cfg, pretrain_init=init).to(DEV).to(dtype)
    x = [t.to(DEV).to(dtype) for t in mc.level_inputs(3, 384, [(5, 3), (1, 2)])]
    with torch.no_grad():
        with pytest.raises(RuntimeError, match='effdet_sepconv_meta failed with code -22'):
            mh(x)
    torch.cuda.synchronize()
    c = _forward_case.__wrapped__(64, dtype, 'main')      # a fresh F = 64 run after the refusal, not the cached one
    _check('F64 outputs after the refusal', c['outs'], c['ro'], dtype)


@pytest.mark.parametrize('first_order', [False, True], ids=['primitives', 'first_order'])
@pytest.mark.parametrize('f', [88, 288])
def test_differentiable_path(f, first_order):
    """grad-enabled forward, d loss / d (every parameter, every input level) and - on the primitives - the Hessian-vector product,
    against float64 autograd through the oracle; metrics, floors and bounds of tests/test_model_gpu.py's two gradient tests"""
    seed = mc.MAIN_SEED[f]
    ro, ra, rg, rhv = _grad_reference(f)
    cfg, mh = _module(f, seed, torch.float32)
    mh.first_order = first_order
    names = [n for n, _ in mh.named_parameters()]
    params = list(mh.parameters())
    assert set(names) == {n for n in rg if not n.startswith('x')}
    xs = [t.to(DEV).requires_grad_() for t in mc.level_inputs(seed, f, mc.GRAD_LEVELS)]
    cot = mc.grad_cotangents(f, 9, mc.GRAD_LEVELS, names, [p.shape for p in params])
    fwd = lambda x_, ret_activs: mh(x_, ret_activs=ret_activs)
    outs, acts, g, hv = mc.first_and_second_order(fwd, names, params, xs, cot, second=not first_order)
    torch.cuda.synchronize()
    _check('F%d grad-mode outputs' % f, outs, ro, torch.float32)
    _check('F%d grad-mode activations' % f, acts, ra, torch.float32)
    eg = mc.grad_error(g, rg, 1e-5, 1e-4)
    print('F%d first_order=%s gradients: worst %s' % (f, first_order, eg[:4]))
    assert eg[0][0] <= 2e-3, eg[:6]
    if not first_order:
        eh = mc.grad_error(hv, rhv, 1e-3)
        print('F%d Hessian-vector product: worst %s' % (f, eh[:4]))
        assert eh[0][0] <= 5e-3, eh[:6]


@functools.lru_cache(maxsize=None)
def _grad_reference(f):
    return mc.oracle_grads(mc.NAME_OF[f], mc.MAIN_SEED[f], mc.GRAD_LEVELS, torch.float64)


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_IDS)
@pytest.mark.parametrize('hw', mc.STAT_SHAPES, ids=['12x20', '1x1'])
def test_layer_batch_statistics(hw, dtype):
    """One layer whose convolution is the identity (centre tap 1, pointwise = I, bias 0) on channels mean + std * normal, mean in
    {0, 1, 8}, std in {1, 0.1, 0.01}; BN weight 1, bias 0.  scale / shift from effdet_bn_batch_stats against 1 / sqrt(var64(Y) +
    eps) and -mean64(Y) scale64 of the output Y the kernel itself wrote (bf16: the rounded values, whose statistics the kernel
    takes on purpose), so the convolution's rounding is no part of the comparison."""
    import _hip
    F_ = mc.STAT_F
    x = mc.stat_input(hw, dtype).to(DEV).permute(0, 2, 3, 1).contiguous()
    taps = torch.zeros(9, F_, dtype=torch.float32, device=DEV); taps[4] = 1.0
    pw = torch.eye(F_, dtype=dtype, device=DEV)
    zero, one = torch.zeros(1, F_, dtype=torch.float32, device=DEV), torch.ones(1, F_, dtype=torch.float32, device=DEV)
    y, scale, shift = _hip.meta_layer_with_stats([x], taps, pw, zero[0].clone(), one, zero, eps=mc.STAT_EPS)
    torch.cuda.synchronize()
    yc = y[0].permute(0, 3, 1, 2).cpu()
    assert float((yc.double() - x.permute(0, 3, 1, 2).cpu().double()).abs().max()) <= 1e-5 * 8.0       # the layer is the identity
    es, et = mc.stat_errors(scale[0], shift[0], yc)
    cells = {}
    for ch in range(F_):
        k = mc.stat_cell(ch)
        cells[k] = (max(cells.get(k, (0, 0))[0], float(es[ch])), max(cells.get(k, (0, 0))[1], float(et[ch])))
    for k, (a, b) in cells.items():
        print('%s %s mean %g std %g: scale %.2e shift %.2e (bound %.1e)' % (hw, dtype, k[0], k[1], a, b, mc.STAT_BOUND))
    assert float(es.max()) <= mc.STAT_BOUND and float(et.max()) <= mc.STAT_BOUND, cells
