#!/usr/bin/env python
"""csrc/energy_reg.hip without a GPU: the unit compiled by g++ against the CPU model of common.h and driven through its C ABI on
numpy arrays - both forms and both energy kinds at C in {1, 7, 65, 90, 129}, T in {1, 2.5}, 1 .. 67 rows and one call of 2100 rows
(two partial workgroups), with and without the filter, float32 and bfloat16 - against the restatement of tests/_energy_reg_ref.py.
It checks arithmetic, indexing and bounds (a guard region follows every buffer), not timing or the memory model.

    python3 tools/simt_model/run_energy_reg.py    needs g++ with C++20 (std::barrier); a thread per lane: about five minutes"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _energy_reg_ref as R  # noqa: E402
from _model import GUARD, build, guarded, ptr  # noqa: E402

FILL = -12345.5


def bf16_round(x):
    """float32 -> bfloat16 bits, round to nearest even (finite values)"""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def call(lib, z, role, form, kind='logsumexp', T=1.0, m_in=None, m_out=None, w_in=1.0, w_out=1.0, min_max=None, phi=(1.0, 0.0),
         want_energy=True, want_grad=True):
    """z [B, N, C] float32 or uint16 (bfloat16 bits), role [B, N] int8 -> the outputs; every guard region is checked"""
    B, N, C = z.shape
    bf16 = z.dtype == np.uint16
    loss, _l = guarded((1,), np.float32, FILL)
    stats, _s = guarded((8,), np.float64, FILL)
    gphi, _g = guarded((2,), np.float32, FILL)
    energy, _e = guarded((B, N), np.float32, FILL)
    gz, _z = guarded((B, N, C), np.uint16 if bf16 else np.float32, 0x5555 if bf16 else FILL)
    ph = np.array(phi, np.float32)
    nbytes = lib.effdet_energy_reg_workspace_bytes(B * N)
    assert nbytes > 0
    ws = np.full(nbytes + GUARD, 0xA5, np.uint8)
    args = (None, 1 if bf16 else 0, ptr(z), ptr(role), B, N, C, R.FORMS.index(form), R.KINDS.index(kind), T, m_in or 0.0, m_out or 0.0, w_in,
            w_out, int(min_max is not None), float(min_max or 0.0), ptr(ph) if form == 'logistic' else None, ptr(loss), ptr(stats),
            ptr(energy) if want_energy else None, ptr(gz) if want_grad else None, ptr(gphi), ptr(ws))
    rc = lib.effdet_energy_reg(*args, nbytes)
    assert rc == 0, rc
    assert (ws[nbytes:] == 0xA5).all(), 'a write beyond the workspace'
    assert (_l[1:] == FILL).all() and (_s[8:] == FILL).all() and (_g[2:] == FILL).all() and (_e[B * N:] == FILL).all(), 'a write beyond an output'
    assert (_z[B * N * C:] == (0x5555 if bf16 else FILL)).all(), 'a write beyond grad_logits'
    if not want_energy:
        assert (energy == FILL).all()
    if not want_grad:
        assert (gz == (0x5555 if bf16 else FILL)).all()
    assert lib.effdet_energy_reg(*args, nbytes - 256) == -22
    return {'loss': loss[0], 'stats': stats.copy(), 'grad_phi': gphi.copy(), 'energy': energy.copy(), 'grad_logits': gz.copy()}


def same(a, b):
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)) for k in a)


def check(got, ref, f32, name, w_in, w_out):
    bnd = R.bounds(ref, f32, w_in, w_out)
    n = ref['side'].shape[0]
    worst = 0.0
    for k, dev in (('energy', got['energy'].reshape(n)), ('grad_logits', got['grad_logits'].reshape(n, -1)), ('grad_phi', got['grad_phi']),
                   ('loss', got['loss']), ('mean_l_in', got['stats'][2]), ('mean_l_out', got['stats'][3]),
                   ('mean_energy_in', got['stats'][4]), ('mean_energy_out', got['stats'][5])):
        err = float(np.abs(np.asarray(dev, np.float64) - ref[k]).max())
        assert err <= bnd[k][1], (name, k, err, bnd[k])
        worst = max(worst, err / bnd[k][1] if bnd[k][1] else 0.0)
    assert [int(v) for v in got['stats'][[0, 1]]] == [ref['n_in'], ref['n_out']], name
    act = R.active_ranges(ref, bnd['energy'][1])                 # exact but for the one row a median margin puts on the kink
    for i, side in ((6, 'in'), (7, 'out')):
        assert act[side][0] <= int(got['stats'][i]) <= act[side][1] <= act[side][0] + 1, (name, side, got['stats'][i], act[side])
    assert not got['energy'].reshape(n)[ref['side'] == 0].any() and not got['grad_logits'].reshape(n, -1)[ref['side'] == 0].any(), name
    return worst


def run(lib, C, form, kind, T):
    worst = 0.0
    for rows, B in ((1, 1), (15, 3), (16, 1), (17, 1), (67, 1), (2100, 2)):
        if rows == 2100 and C > 7:
            continue
        z, role = R.inputs(C, rows)
        E = R.energy(z, kind, T)[0]
        for min_max in (None, float(np.median(z.max(1)))):
            kw = dict(form=form, kind=kind, T=T, w_in=0.75, w_out=1.5, min_max=min_max, phi=(0.5, -1.25),
                      m_in=float(np.float32(np.median(E[role == 1]))) if (role == 1).any() else 0.0,
                      m_out=float(np.float32(np.median(E[role == 0]))) if (role == 0).any() else 0.0)
            ref, f32 = R.forward(z, role, **kw), R.forward(z, role, dtype=np.float32, **kw)
            zz, rr = z.reshape(B, rows // B, C), role.reshape(B, rows // B)
            got = call(lib, zz, rr, **kw)
            name = 'C %d %s %s T %.1f rows %d min_max %r' % (C, form, kind, T, rows, min_max)
            worst = max(worst, check(got, ref, f32, name, 0.75, 1.5))
            if rows in (17, 67):
                # without the optional outputs the others keep their bits; a NaN in a row that does not count changes nothing
                part = call(lib, zz, rr, want_energy=False, want_grad=False, **kw)
                assert all(np.array_equal(part[k], got[k]) for k in ('loss', 'stats', 'grad_phi')), name
                poisoned = zz.copy()
                poisoned.reshape(rows, C)[ref['side'] == 0] = np.nan
                assert same(call(lib, poisoned, rr, **kw), got), name
                # bfloat16 logits against their float32 widening: the same bits, grad_logits after rounding to bfloat16
                bits = (zz.view(np.uint32) >> 16).astype(np.uint16)
                gb, gw = call(lib, bits, rr, **kw), call(lib, R.widen_bf16(bits), rr, **kw)
                assert all(np.array_equal(gb[k], gw[k]) for k in ('loss', 'stats', 'grad_phi', 'energy')), name
                assert np.array_equal(gb['grad_logits'], bf16_round(gw['grad_logits'])), name
    # every role -1; logits of +-80 in counted rows stay finite; a NaN in a counted row: a NaN loss, the other rows keep their bits
    z, role = R.inputs(C, 20)
    kw = dict(form=form, kind=kind, T=T, m_in=-1.0, m_out=-3.0, phi=(0.5, -1.25))
    none = call(lib, z[None], np.full((1, 20), -1, np.int8), **kw)
    assert none['loss'] == 0 and not none['stats'].any() and not none['grad_logits'].any() and not none['energy'].any() and not none['grad_phi'].any()
    role[:4] = (1, 0, 1, 0)
    ext = z.copy()
    ext[0], ext[1], ext[2], ext[3] = 80.0, -80.0, -80.0, 80.0
    a = call(lib, ext[None], role[None], **kw)
    assert all(np.isfinite(a[k]).all() for k in a), {k: np.isfinite(a[k]).all() for k in a}
    ext2 = ext.copy()
    ext2[2, C // 2] = np.nan
    b = call(lib, ext2[None], role[None], **kw)
    keep = np.arange(20) != 2
    assert np.isnan(b['loss']) and np.array_equal(a['energy'][0, keep].view(np.uint32), b['energy'][0, keep].view(np.uint32))
    assert np.array_equal(a['grad_logits'][0, keep].view(np.uint32), b['grad_logits'][0, keep].view(np.uint32))
    print('C %4d, %-8s %-9s T %.1f: ok; worst error / bound %.2f' % (C, form, kind, T, worst))


def refusals(lib):
    z = np.zeros((1, 4, 7), np.float32)
    role = np.zeros((1, 4), np.int8)
    f, d, ph = np.zeros(8, np.float32), np.zeros(8, np.float64), np.zeros(2, np.float32)
    gz = np.zeros((1, 4, 7), np.float32)
    nbytes = lib.effdet_energy_reg_workspace_bytes(4)
    ws = np.zeros(nbytes, np.uint8)

    def go(dtype=0, B=1, N=4, C=7, form=1, kind=0, T=1.0, m_in=0.0, m_out=0.0, w_in=1.0, w_out=1.0, use_min=0, mm=0.0, phi=ptr(ph), loss=ptr(f),
           nb=nbytes):
        return lib.effdet_energy_reg(None, dtype, ptr(z), ptr(role), B, N, C, form, kind, T, m_in, m_out, w_in, w_out, use_min, mm, phi, loss, ptr(d),
                                     None, ptr(gz), ptr(f), ptr(ws), nb)
    assert go() == 0 and go(form=0, phi=None) == 0
    for kw in (dict(dtype=2), dict(B=0), dict(N=0), dict(C=0), dict(C=1025), dict(form=2), dict(kind=2), dict(T=0.0), dict(T=float('nan')),
               dict(kind=1, T=2.0), dict(form=0, m_in=float('inf')), dict(phi=None), dict(w_in=float('nan')), dict(use_min=1, mm=float('nan')),
               dict(loss=None), dict(nb=nbytes - 1), dict(B=1 << 14, N=1 << 14)):
        assert go(**kw) == -22, kw
    q = lib.effdet_energy_reg_workspace_bytes
    assert q(0) == -22 and q((1 << 27) + 1) == -22 and 0 < q(1) <= q(100)
    print('refusals ok')


def main():
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(tmp, 'energy_reg', 'effdet_energy_reg')
        refusals(lib)
        for C in (1, 7, 65, 90, 129):
            for form in R.FORMS:
                for kind, T in (('logsumexp', 1.0), ('logsumexp', 2.5), ('joint', 1.0)):
                    if C in (1, 65, 129) and T == 2.5:
                        continue
                    run(lib, C, form, kind, T)
    print('energy_reg on the CPU model: all checks passed')


if __name__ == '__main__':
    main()
