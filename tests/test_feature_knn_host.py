"""Host-side checks of the nearest-neighbour feature OOD score (ood_features.KNNFeatureOOD, csrc/feature_knn.hip): the C ABI and
every refusal that needs no GPU, the numpy restatement of tests/_feature_knn_ref.py against a brute-force argsort, its
sample_every / capacity bookkeeping across arbitrary splits into calls, and the exclusion cap of the GPU test's nearest-row
comparison on that test's own cases."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _feature_knn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('effdet_feature_knn_workspace_bytes', 'effdet_feature_knn_append', 'effdet_feature_knn_score')
WIDTHS = (64, 88, 112, 160, 224, 288)


def test_entry_points_declared_bound_and_exported():
    from ood_object_detection_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'effdet_hip.h')).read()
    lib = _lib.load()
    for name in NAMES:
        m = re.search(r'\b%s\s*\(([^;]*)\);' % name, header)
        assert m, name
        assert len(_lib.SIGNATURES[name][1]) == m.group(1).count(',') + 1, name
        assert hasattr(lib, name), name
    mk = open(os.path.join(_lib.CSRC, 'Makefile')).read()
    assert 'build/feature_knn.o' in mk and re.search(r'EXTRA_feature_knn\s*=\s*-ffp-contract=off', mk)
    assert re.search(r'build/feature_ood\.o build/feature_knn\.o:\s*feature_rows\.h', mk)
    # the row addressing is stated once, in the shared header
    csrc = _lib.CSRC
    for unit in ('feature_ood.hip', 'feature_knn.hip'):
        src = open(os.path.join(csrc, unit)).read()
        assert '#include "feature_rows.h"' in src and 'fo_row(const FoLevels' not in src, unit
    # so are the ordered compaction and the reductions, in compact.h: no unit defines a count or a base kernel of its own
    assert re.search(r'build/feature_ood\.o build/feature_knn\.o:\s*feature_rows\.h compact\.h', mk)
    assert re.search(r'build/ood_eval\.o:\s*compact\.h', mk)
    assert '#include "compact.h"' in open(os.path.join(csrc, 'feature_rows.h')).read()
    for unit in ('feature_ood.hip', 'feature_knn.hip', 'feature_subspace.hip', 'logit_ood.hip', 'ood_eval.hip'):
        src = open(os.path.join(csrc, unit)).read()
        assert not re.search(r'void \w+_(count|base)_kernel\(', src) and 'block_sum(T v' not in src and 'oe_block_sum' not in src, unit
    assert '#include "compact.h"' in open(os.path.join(csrc, 'ood_eval.hip')).read()
    # the radix sort is stated once, in radix_sort.h, and the integer helpers once, in compact.h
    for unit in ('ood_eval', 'eval_scale'):
        src = open(os.path.join(csrc, unit + '.hip')).read()
        assert '#include "radix_sort.h"' in src and not re.search(r'void \w+_sort_(hist|scan|scatter)_kernel\(', src), unit
        assert re.search(r'build/%s\.o:.*\bcompact\.h.*\bradix_sort\.h' % unit, mk), unit
    src = open(os.path.join(csrc, 'eval_scale.hip')).read()
    assert not re.search(r'\w+_block_excl_scan\(unsigned v|unsigned \w+_(key|floor_pow2|min|popc)\(', src)
    # the candidate search and the IoU of the two matchers once, in eval_match.h
    for unit in ('evaluation', 'eval_scale'):
        src = open(os.path.join(csrc, unit + '.hip')).read()
        assert '#include "eval_match.h"' in src and '__shfl_xor(bj' not in src and 'inter / (' not in src, unit
        assert re.search(r'build/%s\.o:.*\beval_match\.h' % unit, mk), unit


def _table(n=1, cells=(100,), channel=1, F=64):
    lls = lambda v: (ctypes.c_longlong * len(v))(*v)
    buf = ctypes.create_string_buffer(64)
    base = ctypes.addressof(buf)
    return buf, (n, (ctypes.c_void_p * len(cells))(*[base] * len(cells)), lls(cells), lls([c * F for c in cells]), lls([F] * len(cells)),
                 lls([channel] * len(cells)))


def test_argument_refusals_before_any_launch():
    """every call below must return -22 from pure host code: this machine has no GPU to launch on"""
    from ood_object_detection_amd import _lib
    lib = _lib.load()
    q = lib.effdet_feature_knn_workspace_bytes
    assert 0 < q(1, 64, 0, 0) < q(1 << 27, 64, 0, 0)                                 # append
    assert 0 < q(100, 64, 1, 1) < q(100, 64, 10, 1) < q(100, 64, 10, 7) <= q(100, 64, 10, 0)
    assert q(6400, 64, 10, 0) < q(6400, 64, 10, 64) and q(1 << 27, 288, 32, 64) > 0
    for bad in ((0, 64, 10, 1), ((1 << 27) + 1, 64, 10, 1), (100, 96, 10, 1), (100, 0, 10, 1), (100, 64, -1, 1), (100, 64, 33, 1),
                (100, 64, 10, -1), (100, 64, 10, 65)):
        assert q(*bad) == -22, bad
    buf, ok = _table()
    p = ctypes.addressof(buf)                                 # any non-null address: nothing is dereferenced on the host

    def append(table=ok, dtype=0, F=64, C=3, A=9, B=1, K=10, cdt=1, classes=p, every=1, cap=1000, ws=1 << 30):
        return lib.effdet_feature_knn_append(None, dtype, *table, F, C, A, B, K, None, classes, cdt, K, 1, 0, None, 0, 1, every, cap, p, p, p, p,
                                             p, ws)

    def score(table=ok, dtype=0, F=64, A=9, B=1, K=10, k=10, splits=0, M=100, ws=1 << 30):
        return lib.effdet_feature_knn_score(None, dtype, *table, F, A, B, K, None, None, 0, 1, k, splits, M, p, p, p, p, p, p, p, ws)

    for fn in (append, score):
        assert fn(F=96) == -22 and fn(F=0) == -22                                   # an unsupported width
        assert fn(table=_table(channel=2)[1]) == -22                                # a channel stride other than 1
        assert fn(table=_table(n=9, cells=(10,) * 9)[1]) == -22                     # more than 8 levels
        assert fn(table=_table(n=0)[1]) == -22 and fn(table=_table(cells=(0,))[1]) == -22
        assert fn(A=0) == -22 and fn(B=0) == -22 and fn(K=0) == -22 and fn(B=1 << 14, K=1 << 14) == -22
        assert fn(dtype=2) == -22                                                   # float32 or bfloat16 features only
        assert fn(ws=8) == -22                                                      # a workspace too small
    assert append(C=-1) == -22 and append(cdt=3) == -22 and append(classes=None) == -22
    assert append(every=0) == -22 and append(cap=0) == -22 and append(cap=(1 << 24) + 1) == -22
    assert score(k=0) == -22 and score(k=33) == -22 and score(splits=-1) == -22 and score(splits=65) == -22
    assert score(M=0) == -22 and score(M=(1 << 24) + 1) == -22


def test_python_refusals():
    from ood_object_detection_amd import ood_features as of
    K = of.KNNFeatureOOD
    for kw in (dict(num_features=96), dict(k=0), dict(k=33), dict(capacity=0), dict(capacity=(1 << 24) + 1), dict(sample_every=0),
               dict(num_classes=0), dict(num_anchors=0)):
        with pytest.raises(ValueError):
            K(**dict(dict(num_features=64, num_anchors=9, capacity=100), **kw))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        K(64, 9, 100, device='cpu')
    f = K(64, 9, 100)                                         # nothing touches the device before the first add
    x = torch.zeros(2, 50, 64)
    with pytest.raises(RuntimeError, match='fit'):
        f.score(x, torch.zeros(2, 4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        f.add(x)
    with pytest.raises(ValueError):
        f.fit(k=40)
    # two scorers that write the same keys are refused at construction
    from ood_object_detection_amd.effdet import bench
    with pytest.raises(ValueError, match='knn'):
        bench._feature_scorers([f, K(64, 9, 10)])
    assert bench._feature_scorers(None) == () and bench._feature_scorers(f) == (f,)
    assert len(bench._feature_scorers([of.FeatureOOD(64, 3, 9), f])) == 2


def test_restatement_against_brute_force():
    rs = np.random.RandomState(5)
    for normalize in (False, True):
        for M, k in ((1, 3), (4, 4), (9, 1), (9, 5)):
            bank, q = rs.normal(size=(M, 8)).astype(np.float32), rs.normal(size=(6, 8)).astype(np.float32)
            if M > 4:
                bank[7] = bank[2]                                                   # a tie in value: the lower row wins
                q[0] = bank[2]
            y = rs.randint(0, 3, M)
            got = R.score(q, bank, k, normalize, y)
            b64, q64 = bank.astype(np.float64), q.astype(np.float64)
            if normalize:
                b64, q64 = b64 / np.linalg.norm(b64, axis=1, keepdims=True), q64 / np.linalg.norm(q64, axis=1, keepdims=True)
            d2 = ((q64[:, None, :] - b64[None, :, :]) ** 2).sum(2)
            order = np.argsort(d2, 1, kind='stable')
            kth = np.take_along_axis(d2, order, 1)[:, min(k, M) - 1]
            assert np.abs(-got['knn'] - kth).max() <= 1e-12 * max(d2.max(), 1.0)
            assert np.array_equal(got['index'][1:], order[1:, 0]) and np.array_equal(got['cls'], y[got['index']])
            if M > 4:
                assert got['index'][0] == 2 and got['gap'][0] <= 1e-12 and (k > 1 or abs(got['knn'][0]) <= 1e-12)
    # the summation order of |x|^2 does not matter in float64 beyond rounding, and is the stated one in float32
    x = rs.normal(size=(5, 88)).astype(np.float32)
    assert np.abs(R.sumsq(x) - (x.astype(np.float64) ** 2).sum(1)).max() <= 1e-12
    p = np.zeros((5, 16), np.float32)
    for c in range(0, 96, 16):
        blk = np.zeros((5, 16), np.float32)
        blk[:, :min(16, 88 - c)] = x[:, c:c + 16]
        p = p + blk * blk
    want = ((p[:, 0] + p[:, 8]) + (p[:, 4] + p[:, 12]) + ((p[:, 2] + p[:, 10]) + (p[:, 6] + p[:, 14]))) + \
           ((p[:, 1] + p[:, 9]) + (p[:, 5] + p[:, 13]) + ((p[:, 3] + p[:, 11]) + (p[:, 7] + p[:, 15])))
    assert np.array_equal(R.sumsq(x, np.float32), want)


@pytest.mark.parametrize('every,capacity', [(1, 10000), (3, 10000), (1, 300), (4, 150), (7, 1)])
def test_bank_bookkeeping_does_not_depend_on_the_split_into_calls(every, capacity):
    rs = np.random.RandomState(every + capacity)
    x, y = rs.normal(size=(1000, 16)).astype(np.float32), rs.randint(0, 5, 1000)
    whole = R.Bank(16, capacity, True, every)
    whole.add(x, y)
    kept = np.arange(1000)[::every]
    assert whole.seen == 1000 and whole.size == min(len(kept), capacity) and whole.lost == len(kept) - whole.size
    assert np.array_equal(whole.classes, y[kept][:capacity])
    for trial in range(4):
        cuts = np.sort(rs.randint(0, 1001, rs.randint(1, 9)))
        parts = R.Bank(16, capacity, True, every)
        for lo, hi in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [1000]])):
            parts.add(x[lo:hi], y[lo:hi])                                           # empty calls included
        assert (parts.size, parts.seen, parts.lost) == (whole.size, whole.seen, whole.lost)
        assert np.array_equal(parts.rows.view(np.uint32), whole.rows.view(np.uint32)) and np.array_equal(parts.classes, whole.classes)
        assert np.array_equal(parts.norms.view(np.uint32), whole.norms.view(np.uint32))
    whole.clear()
    assert (whole.size, whole.seen, whole.lost) == (0, 0, 0)


@pytest.mark.parametrize('normalize', [True, False])
@pytest.mark.parametrize('F,C', [(F, C) for F in WIDTHS for C in (1, 90)])
def test_exclusion_cap_of_the_nearest_row_comparison(F, C, normalize):
    """The GPU test compares knn_index exactly outside the rows whose float64 gap between the nearest and the second-nearest d2
    is at most twice the value bound.  On every case that test uses (4096 bank rows, 2000 in and 2000 OOD queries) that share is
    at most 1 % - checked here, without a device, for the in and the OOD queries separately and every k."""
    c = R.case(F, C, normalize)
    for k in R.KS:
        ref, e32, bnd = c[k]
        ex = R.excluded(ref, bnd)
        shares = (ex[:R.N_Q].mean(), ex[R.N_Q:].mean())
        print('F %d C %d normalize %d k %d: E32 %.2e, bound %.2e, max d2 %.3g, excluded in %d, OOD %d of %d'
              % (F, C, normalize, k, e32, bnd, ref['max_d2'], ex[:R.N_Q].sum(), ex[R.N_Q:].sum(), R.N_Q))
        assert max(shares) <= 0.01, shares
