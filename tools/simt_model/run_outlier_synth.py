#!/usr/bin/env python
"""csrc/outlier_synth.hip without a GPU: the unit compiled by g++ against the CPU model of common.h and driven through its C ABI on
numpy arrays - the norms, the four passes of the shared radix sort, the finish, rows and advance launches at F in {8, 64, 88},
S in {1, 63, 65, 300} (one and two workgroups of candidates), k from 1 to S, a class list with an invalid and an out-of-range class -
against the restatement of tests/_outlier_synth_ref.py under its bound.  It checks arithmetic, indexing and bounds (a guard region
follows every buffer), not timing or the memory model.

    python3 tools/simt_model/run_outlier_synth.py    needs g++ with C++20 (std::barrier); a thread per lane: a few minutes"""
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _outlier_synth_ref as R  # noqa: E402
from _model import GUARD, build, guarded, ptr  # noqa: E402

FILL = -12345.5


def call(lib, F, C, ids, S, k, seed, t, mu, L, valid, advance=1):
    """-> the outputs of one call; every guard region is checked"""
    n = C if ids is None else len(ids)
    mu32 = np.ascontiguousarray(mu, np.float32)
    U = np.ascontiguousarray(np.asarray(L).T, np.float32)
    cst = np.array([R.log_const(L)], np.float32)
    val = np.ascontiguousarray(valid, np.int8)
    draw = np.array([t], np.int64)
    idl = None if ids is None else np.ascontiguousarray(ids, np.int32)
    outs = {'rows': guarded((n, k, F), np.float32, FILL), 'index': guarded((n, k), np.int32, -77), 'r2': guarded((n, k), np.float32, FILL),
            'log_density': guarded((n, k), np.float32, FILL), 'roles': guarded((n * k,), np.int8, 55)}
    nbytes = lib.effdet_outlier_synth_workspace_bytes(n, S)
    assert nbytes > 0
    ws = np.full(nbytes + GUARD, 0xA5, np.uint8)
    args = (None, F, C, n, ptr(idl), S, k, seed, ptr(draw), advance, ptr(mu32), ptr(U), ptr(cst), ptr(val)) + tuple(
        ptr(outs[key][0]) for key in ('rows', 'index', 'r2', 'log_density', 'roles')) + (ptr(ws),)
    assert lib.effdet_outlier_synth(*args, nbytes - 256) == -22
    rc = lib.effdet_outlier_synth(*args, nbytes)
    assert rc == 0, rc
    assert (ws[nbytes:] == 0xA5).all(), 'a write beyond the workspace'
    for key, fill in (('rows', FILL), ('index', -77), ('r2', FILL), ('log_density', FILL), ('roles', 55)):
        view, whole = outs[key]
        assert (whole[view.size:] == fill).all(), 'a write beyond ' + key
    assert int(draw[0]) == t + (1 if advance else 0)
    return {key: v[0].copy() for key, v in outs.items()}


def check(lib, F, C, S, k, seed, t, ids=None, invalid=()):
    mu, L = R.gaussians(F, C, seed=F + C)
    valid = np.ones(C, bool)
    valid[list(invalid)] = False
    got = call(lib, F, C, ids, S, k, seed, t, mu, L, valid)
    classes = list(range(C)) if ids is None else list(ids)
    real = [c if 0 <= c < C else None for c in classes]
    worst = 0.0
    for ci, c in enumerate(real):
        ok = c is not None and valid[c]
        assert (got['roles'][ci * k:(ci + 1) * k] == (0 if ok else -1)).all()
        if not ok:
            assert not got['rows'][ci].any()
        if c is None:
            continue
        w = R.words(seed, t, c, np.arange(S), F)
        z64, z32 = R.normals(w, np.float64), R.normals(w, np.float32)
        r64, r32 = R.sqnorm(z64), R.sqnorm(z32)
        b_r2 = R.bound(np.abs(r32 - r64).max(), r64)
        idx = got['index'][ci]
        assert len(set(idx.tolist())) == k and idx.min() >= 0 and idx.max() < S
        assert np.abs(got['r2'][ci] - r64[idx]).max() <= b_r2
        d = np.diff(got['r2'][ci])
        assert (d <= 0).all() and (np.diff(idx)[d == 0] > 0).all()
        assert got['r2'][ci][-1] + 2 * b_r2 >= np.delete(r64, idx).max(initial=-np.inf)      # nothing decidedly larger was left out
        assert np.array_equal(got['log_density'][ci], -(got['r2'][ci] * np.float32(0.5)) + np.float32(R.log_const(L)))
        if ok:
            a64, a32 = R.rows(mu[c], L, z64[idx]), R.rows(mu[c], L, z32[idx])
            err, b = np.abs(got['rows'][ci] - a64).max(), R.bound(np.abs(a32 - a64).max(), a64)
            assert err <= b, (err, b)
            worst = max(worst, err / b)
    print('F %3d C %2d S %3d k %3d classes %s: ok (rows at most %.2f of their bound)' % (F, C, S, k, 'all' if ids is None else list(ids), worst), flush=True)
    return got


def main():
    tmp = tempfile.mkdtemp(prefix='simt_outlier_synth_')
    try:
        lib = build(tmp, 'outlier_synth', 'effdet_outlier_synth')
        t = (3 << 32) | 5
        check(lib, 8, 1, 1, 1, 1, 0)
        check(lib, 64, 2, 63, 4, 1, t)
        whole = check(lib, 88, 3, 65, 65, 2, t, invalid=(1,))
        part = check(lib, 88, 3, 65, 65, 2, t, ids=[2, -1, 1, 3, 0], invalid=(1,))
        for key in ('rows', 'index', 'r2', 'log_density'):                                    # any grouping of the classes: the same bits
            assert np.array_equal(part[key][0], whole[key][2]) and np.array_equal(part[key][4], whole[key][0]), key
        check(lib, 64, 2, 300, 16, (1 << 63) + 12345, 7)
        q = lib.effdet_outlier_synth_workspace_bytes
        assert q(0, 8) == -22 and q(1025, 8) == -22 and q(1, 0) == -22 and q(1, (1 << 20) + 1) == -22 and q(1024, 1 << 17) == -22
        print('outlier_synth on the CPU model: all checks passed')
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    main()
