"""Host checks behind tests/test_meta_head_widths_gpu.py: the float64 MetaHead yardstick is the restatement the fixture pins, the
seeded inputs of every width are well enough conditioned that the project's float32 bound measures the kernel and not the
problem, and the bound of the layer-level statistics test separates a two-pass float32 computation from the one-pass formula
(sum q*q / n - mean^2 on float32 tile sums) by a factor of ten on each side."""
import numpy as np
import pytest
import torch

import _meta_head_cases as mc
from oracle import model as om

WIDTH_IDS = [str(f) for _, f, _ in mc.WIDTHS]


def test_float64_oracle_matches_reference_fixture(golden):
    """the dtype=float64 form against tests/golden/meta_nets.npz, at the fixture's own tolerance (test_oracle_golden.py)"""
    from _seeded import meta_lists, meta_nets_case
    g = golden('meta_nets')
    c = meta_nets_case(g)
    dw, pw, pb, pred, bw, bb = meta_lists(c['init'], c['extra'], c['L'], c['R'])
    tol = lambda a, b: float((a - torch.from_numpy(b).double()).abs().max()) <= 2e-5 * max(1.0, float(np.abs(b).max()))
    o, a = om.meta_head_forward(dw, pw, pb, bw, bb, pred, c['x'], dtype=torch.float64)
    assert all(t.dtype == torch.float64 for t in o + a)
    for i in range(c['L']):
        assert tol(o[i], g['mh_out%d' % i]) and tol(a[i], g['mh_act%d' % i])
    off = int(g['supp_level_offset_default'])
    o4, a4, c4 = om.meta_head_forward(dw, pw, pb, bw, bb, pred, c['x'], level_offset=off, dtype=torch.float64,
                                      predict_class=[c['extra']['predict_pw_sep'], c['extra']['predict_pb_sep']])
    for i in range(c['L'] - off):
        assert tol(c4[i], g['mh_both_cls%d' % i]) and tol(o4[i], g['mh_both_anch%d' % i]) and tol(a4[i], g['mh_both_act%d' % i])
    # the default stays float32
    assert om.meta_head_forward(dw, pw, pb, bw, bb, pred, c['x'])[0][0].dtype == torch.float32


def test_builder_follows_the_configs():
    for name, f, r in mc.WIDTHS:
        cfg = mc.config_of(name)
        assert (cfg.fpn_channels, cfg.box_class_repeats, cfg.num_levels) == (f, r, 5)
    cfg, init, extra, mh = mc.build_meta_head('tf_efficientdet_d1', 3, sep_head=True)
    dw, pw, pb, pred, bw, bb = mc.head_lists(cfg, init, extra)
    same = lambda ps, ts: len(ps) == len(ts) and all(torch.equal(p.detach(), t) for p, t in zip(ps, ts))
    assert same(mh.conv_dw_rep, dw) and same(mh.conv_pw_rep, pw) and same(mh.conv_pb_rep, pb) and same(mh.predict, pred)
    assert same(mh.bn_rep_w, bw) and same(mh.bn_rep_b, bb)
    assert same(mh.predict_class, [extra['predict_pw_sep'], extra['predict_pb_sep']])
    assert abs(float(torch.stack(bw).mean()) - 1.0) < 0.05 and 0.15 < float(torch.stack(bw).std()) < 0.25


def _oracle_gap(name, f, seed, levels):
    cfg, init, extra = mc.head_weights(name, seed)
    x = mc.level_inputs(seed, f, levels)
    o64, o32 = mc.oracle(cfg, init, extra, x, torch.float64), mc.oracle(cfg, init, extra, x, torch.float32)
    return max(mc.f32_error(a, b) for a, b in zip(o32[0] + o32[1], o64[0] + o64[1])), (cfg, init, extra, x)


@pytest.mark.parametrize('name,f,r', mc.WIDTHS, ids=WIDTH_IDS)
def test_main_inputs_are_well_conditioned(name, f, r):
    """float32 on the CPU stays within a tenth of the float32 bound of float64, and no (level, layer) has a channel whose batch
    variance is below 1e-3: an error above the bound on the GPU is the kernel's"""
    seed = mc.MAIN_SEED[f]
    assert mc.SEED_BASE <= seed < mc.SEED_BASE + mc.SEED_TRIES
    gap, (cfg, init, extra, x) = _oracle_gap(name, f, seed, mc.MAIN_LEVELS)
    low = mc.min_batch_variance(cfg, init, extra, x)
    print('F %d seed %d: float32 vs float64 oracle %.2e, smallest batch variance %.2e' % (f, seed, gap, low))
    assert gap <= 0.1 * mc.F32_BOUND
    assert low >= 1e-3


@pytest.mark.parametrize('name,f,r', mc.WIDTHS, ids=WIDTH_IDS)
def test_few_sample_inputs_are_well_conditioned(name, f, r):
    """the same float32-against-float64 condition with 4 and 2 samples per channel, where torch float32 itself can lose the bound"""
    seed, levels = mc.FEW_CASE[f]
    assert mc.SEED_BASE <= seed < mc.SEED_BASE + mc.SEED_TRIES
    assert levels in (mc.FEW_LEVELS, mc.FEW_LEVELS_FALLBACK)
    gap, _ = _oracle_gap(name, f, seed, levels)
    print('F %d seed %d levels %s: float32 vs float64 oracle %.2e' % (f, seed, levels, gap))
    assert gap <= 0.1 * mc.F32_BOUND


def _per_cell(err):
    cells = {}
    for c in range(mc.STAT_F):
        k = mc.stat_cell(c)
        cells[k] = max(cells.get(k, 0.0), float(err[c]))
    return cells


def test_statistics_yardstick_discriminates():
    """On the exact inputs of the layer-level GPU test: float32 two-pass statistics are ten times below STAT_BOUND on every cell
    and shape, and the one-pass formula is ten times above it, at n = 480, on the cells whose mean is at least 80 standard
    deviations - (1, 0.01), (8, 0.1), (8, 0.01).  (At mean 1 / std 0.1 the one-pass formula loses 4e-6 only - eps * mean^2 / var
    = 6e-6 - which no bound separates from a correct computation by two factors of ten; that cell is printed, not asserted.)"""
    two, one = 0.0, {}
    for hw in mc.STAT_SHAPES:
        y = mc.stat_input(hw)
        assert y.dtype == torch.float32 and tuple(y.shape) == (mc.B, mc.STAT_F) + hw
        worst = torch.maximum(*mc.stat_errors(*mc.stat_two_pass_f32(y), y))
        two = max(two, float(worst.max()))
        for tw in (8, 16):
            cells = _per_cell(torch.maximum(*mc.stat_errors(*mc.stat_one_pass_f32(y, 8, tw), y)))
            print(hw, 'one-pass, 8 x %d tiles:' % tw, {k: '%.1e' % v for k, v in cells.items()})
            if hw == (12, 20) and tw == 8:          # n = 480 in the float32 tiling
                one = cells
    sensitive = [(m, s) for m in mc.STAT_MEANS for s in mc.STAT_STDS if s > 0 and m / s >= 80]
    assert sorted(sensitive) == [(1.0, 0.01), (8.0, 0.01), (8.0, 0.1)]
    low = min(one[k] for k in sensitive)
    print('two-pass float32 worst %.2e, one-pass float32 least sensitive cell %.2e, bound %.1e' % (two, low, mc.STAT_BOUND))
    assert 10.0 * two <= mc.STAT_BOUND
    assert low >= 10.0 * mc.STAT_BOUND
    # every cell and several channels per cell are present
    assert len({mc.stat_cell(c) for c in range(mc.STAT_F)}) == 9


def test_bf16_statistics_inputs_are_exact_for_both_formulas():
    """values already rounded to bf16 have exact float32 squares: both formulas stay ten times below the bound (the bf16 GPU case
    guards the kernel's choice of taking the statistics of the rounded values, not the variance formula)"""
    for hw in mc.STAT_SHAPES:
        y = mc.stat_input(hw, torch.bfloat16)
        for fn in (mc.stat_two_pass_f32, lambda t: mc.stat_one_pass_f32(t, 8, 16)):
            assert 10.0 * float(torch.maximum(*mc.stat_errors(*fn(y), y)).max()) <= mc.STAT_BOUND


@pytest.mark.parametrize('f', [88, 288])
def test_gradient_inputs_are_well_conditioned(f):
    """the differentiable-path case (GRAD_LEVELS): float32 autograd on the CPU is within a fifth of each gradient bound of float64
    (the worst tensor is a conv bias in front of a batch-statistics BN, whose gradient is analytically zero: all of it is
    rounding, measured against the floor), and its outputs within a tenth of the float32 bound"""
    name, seed = mc.NAME_OF[f], mc.MAIN_SEED[f]
    o64, a64, g64, h64 = mc.oracle_grads(name, seed, mc.GRAD_LEVELS, torch.float64)
    o32, a32, g32, h32 = mc.oracle_grads(name, seed, mc.GRAD_LEVELS, torch.float32)
    gap = max(mc.f32_error(a, b) for a, b in zip(o32 + a32, o64 + a64))
    eg = mc.grad_error(g32, g64, 1e-5, 1e-4)
    eh = mc.grad_error(h32, h64, 1e-3)
    print('F %d: outputs %.2e, gradients %.2e (%s), Hessian-vector product %.2e (%s)' % (f, gap, eg[0][0], eg[0][1], eh[0][0], eh[0][1]))
    assert gap <= 0.1 * mc.F32_BOUND
    assert eg[0][0] <= 0.2 * 2e-3, eg[:4]
    assert eh[0][0] <= 0.2 * 5e-3, eh[:4]
    # parameters of levels the case does not feed have no gradient
    assert g64['bn_w04'] is None and g64['bn_w00'] is not None
