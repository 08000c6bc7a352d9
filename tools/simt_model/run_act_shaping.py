#!/usr/bin/env python
"""csrc/act_shaping.hip without a GPU: the unit compiled by g++ against the CPU model of common.h (which models the float32-input
MFMA as the fmaf chain it is) and driven through its C ABI on numpy arrays - entries form, cells form and fit, every method, at
F = 64 and 88, C in {2, 17}, float32 and bfloat16 towers - against the restatement of tests/_act_shaping_ref.py.  It checks
arithmetic, indexing and bounds (a guard region follows every buffer), not timing or the memory model.

    python3 tools/simt_model/run_act_shaping.py     needs g++ with C++20 (std::barrier); a thread per lane: a few minutes"""
import ctypes
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _act_shaping_ref as R  # noqa: E402
from _model import GUARD, build, guarded, ptr  # noqa: E402
from ood_object_detection_amd.ood_shaping import METHODS, pack_head  # noqa: E402

A = 3


def arr(ctype, v):
    return (ctype * len(v))(*[int(x) for x in v])


def table(tower):
    """per-level NHWC arrays (float32, or uint16 bfloat16 bits) -> the level table with heights and widths"""
    es = tower[0].itemsize
    return (0 if es == 4 else 1, len(tower), (ctypes.c_void_p * len(tower))(*[t.ctypes.data for t in tower]),
            arr(ctypes.c_longlong, [t.shape[1] * t.shape[2] for t in tower]), arr(ctypes.c_longlong, [t.strides[0] // es for t in tower]),
            arr(ctypes.c_longlong, [t.strides[2] // es for t in tower]), arr(ctypes.c_longlong, [1] * len(tower)),
            arr(ctypes.c_int, [t.shape[1] for t in tower]), arr(ctypes.c_int, [t.shape[2] for t in tower]))


def check_keys(tag, got, ref, bnd, live, worst):
    for k, g in got.items():
        if k == 'class':
            sure = ref['margin'][live] >= 2 * bnd['logits'][1]
            assert np.array_equal(g[live][sure], ref['class'][live][sure]), (tag, k)
        else:
            err = np.abs(g[live] - ref[k][live]).max()
            assert err <= bnd[k][1], (tag, k, err, bnd[k])
            worst[k] = max(worst.get(k, 0.0), err / bnd[k][1])


def run(lib, F, C, bf16):
    B = 2
    d_in = R.inputs(F, C, A, B)
    tower = d_in['tower']
    if bf16:
        bits = [R.to_bf16_bits(t) for t in tower]
        tower, dev_tower = [R.widen_bf16(b) for b in bits], bits
    else:
        dev_tower = tower
    taps, W, bias = d_in['taps'], d_in['W'], d_in['bias']
    w_rows, w_tiles, bias_p = pack_head(W, bias, A)
    d = R.penultimate(tower, taps)                                       # [B, P, F]
    P = d.shape[1]
    N = A * P
    rs = np.random.RandomState(F + C)
    K = 11
    anchor = np.stack([rs.permutation(N)[:K] for _ in range(B)]).astype(np.int64)
    anchor[1, 3] = N                                                     # outside [0, A * P): does not count
    count = np.array([K, 7], np.int32)
    live = (np.arange(K)[None, :] < count[:, None]) & (anchor < N)
    cell, slot = np.minimum(anchor, N - 1) // A, np.minimum(anchor, N - 1) % A
    d_rows = d[np.arange(B)[:, None], cell].reshape(B * K, F)
    lf = live.ravel()
    c_val = np.float32(np.quantile(d, 0.9))
    c_dev = np.array([c_val], np.float32)
    t = table(dev_tower)
    worst = {}
    for method in METHODS:
        k = R.k_of(F, 90.0) if method in METHODS[2:] else 0
        kw = dict(method=method, k=k, c=c_val, T=1.5, gradnorm=True)
        ref = R.score(d_rows, slot.ravel(), W, bias, A, **kw)
        f32 = R.score(d_rows, slot.ravel(), W, bias, A, dtype=np.float32, **kw)
        bnd = R.bounds({k_: v[lf] for k_, v in ref.items()}, {k_: v[lf] for k_, v in f32.items()})
        (en, _e), (ml, _m), (gn, _g) = (guarded((B, K), np.float32, -12345.5) for _ in range(3))
        cl, _c = guarded((B, K), np.int64, -77)
        xr, _x = guarded((B, K, F), np.float32, -12345.5)
        rc = lib.effdet_act_shaping_score(None, *t, F, C, A, B, K, ptr(anchor), ptr(count), 0, ptr(taps), ptr(w_rows), ptr(bias_p),
                                          METHODS.index(method), k, ptr(c_dev), 1.5, ptr(en), ptr(ml), ptr(cl), ptr(gn), ptr(xr))
        assert rc == 0, rc
        for w_, n_, fill in ((_e, B * K, -12345.5), (_m, B * K, -12345.5), (_g, B * K, -12345.5), (_c, B * K, -77), (_x, B * K * F, -12345.5)):
            assert (w_[n_:] == fill).all(), 'a write beyond an output'
        assert (en[~live] == 0).all() and (ml[~live] == 0).all() and (gn[~live] == 0).all() and (cl[~live] == -1).all() and (xr[~live] == 0).all()
        got = {'energy': en.ravel(), 'max_logit': ml.ravel(), 'gradnorm': gn.ravel(), 'class': cl.ravel()}
        check_keys((F, C, method, 'entries'), got, ref, bnd, lf, worst)
        x32 = f32['rows']
        if method in ('none', 'react', 'ash_p'):
            assert np.array_equal(xr.reshape(B * K, F)[lf].view(np.uint32), x32[lf].view(np.uint32)), (method, 'rows')
        else:
            assert np.array_equal(xr.reshape(B * K, F)[lf] == 0, x32[lf] == 0), (method, 'zero pattern')
        # cells form: every anchor
        all_d, all_slot = np.repeat(d.reshape(B * P, F), A, 0), np.tile(np.arange(A), B * P)
        cref = R.score(all_d, all_slot, W, bias, A, **kw)
        cf32 = R.score(all_d, all_slot, W, bias, A, dtype=np.float32, **kw)
        cb = R.bounds(cref, cf32)
        (en2, _e), (ml2, _m), (gn2, _g) = (guarded((B, N), np.float32, -12345.5) for _ in range(3))
        cl2, _c = guarded((B, N), np.int64, -77)
        rc = lib.effdet_act_shaping_score_cells(None, *t, F, C, A, B, ptr(taps), ptr(w_tiles), ptr(bias_p), METHODS.index(method), k,
                                                ptr(c_dev), 1.5, ptr(en2), ptr(ml2), ptr(cl2), ptr(gn2))
        assert rc == 0, rc
        assert (_e[B * N:] == -12345.5).all() and (_m[B * N:] == -12345.5).all() and (_g[B * N:] == -12345.5).all() and (_c[B * N:] == -77).all()
        got = {'energy': en2.ravel(), 'max_logit': ml2.ravel(), 'gradnorm': gn2.ravel(), 'class': cl2.ravel()}
        check_keys((F, C, method, 'cells'), got, cref, cb, np.ones(B * N, bool), worst)
        # a second image alone: the same bits for its cells
        t1 = table([x[1:] for x in dev_tower])
        en3 = np.zeros((1, N), np.float32)
        ml3, gn3, cl3 = np.zeros_like(en3), np.zeros_like(en3), np.zeros((1, N), np.int64)
        assert lib.effdet_act_shaping_score_cells(None, *t1, F, C, A, 1, ptr(taps), ptr(w_tiles), ptr(bias_p), METHODS.index(method), k,
                                                  ptr(c_dev), 1.5, ptr(en3), ptr(ml3), ptr(cl3), ptr(gn3)) == 0
        assert np.array_equal(en3[0].view(np.uint32), en2[1].view(np.uint32)) and np.array_equal(gn3[0].view(np.uint32), gn2[1].view(np.uint32))
        assert np.array_equal(cl3[0], cl2[1])
    # fit
    nbytes = lib.effdet_act_shaping_workspace_bytes(B * K, F)
    assert nbytes > 0
    ws = np.full(nbytes + GUARD, 0xA5, np.uint8)
    n_, _n = guarded((1,), np.int64, -7)
    sd, _s = guarded((F,), np.float64, -7.5)
    hist, _h = guarded((65536,), np.int64, -7)
    n_[:] = 0
    sd[:] = 0
    hist[:] = 0
    for _ in range(2):
        rc = lib.effdet_act_shaping_fit(None, *t, F, A, B, K, ptr(anchor), ptr(count), 0, ptr(taps), ptr(n_), ptr(sd), ptr(hist), ptr(ws), nbytes)
        assert rc == 0, rc
    assert (ws[nbytes:] == 0xA5).all() and (_n[1:] == -7).all() and (_s[F:] == -7.5).all() and (_h[65536:] == -7).all()
    rn, rsum, rhist = R.fit_stats(d_rows[lf])
    assert int(n_[0]) == 2 * rn and np.array_equal(hist, 2 * rhist)
    assert np.abs(sd - 2 * rsum).max() <= 1e-12 * np.abs(d_rows[lf].astype(np.float64)).sum(0).max() * 2
    assert lib.effdet_act_shaping_fit(None, *t, F, A, B, K, ptr(anchor), ptr(count), 0, ptr(taps), ptr(n_), ptr(sd), ptr(hist), ptr(ws),
                                      nbytes - 256) == -22
    print('F %3d C %3d %s: entries, cells and fit ok; worst error / bound: %s'
          % (F, C, 'bf16' if bf16 else 'f32 ', ', '.join('%s %.2f' % kv for kv in sorted(worst.items()))))


def main():
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(tmp, 'act_shaping', 'effdet_act_shaping_')
        assert lib.effdet_act_shaping_workspace_bytes(0, 64) == -22 and lib.effdet_act_shaping_workspace_bytes(4, 65) == -22
        for F, C, bf16 in ((64, 2, False), (88, 17, False), (64, 17, True)):
            run(lib, F, C, bf16)
    print('act_shaping on the CPU model: all checks passed')


if __name__ == '__main__':
    main()
