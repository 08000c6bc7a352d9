"""The ordered compaction of csrc/compact.h at its tile (2048 entries) and wave-round (64 / 512 entries) edges, through the four
units that use it: FeatureOOD.add, KNNFeatureOOD.add, LogitOOD.add and OODEvaluator's append.

Reference-free and exact.  A [B, K] call of which only some entries count must leave what a dense call holding just those entries,
in (b, j) order, leaves: the units state that positions (and with them every summation order) depend on nothing but the number of
kept entries.  Totals B * K of 513, 2047, 2048 and 2049 with B = 1, and 513 and 2049 with B = 3; kept: all, none, every third, the
last entry alone, and the entries on either side of a wave round, a wave's share and a tile.  An entry is dropped through its
class (outside [0, C)), through a max logit below the threshold or a detection score below the minimum, and - behind the last kept
entry of an image - through `count` as well."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F = 64
SHAPES = ((1, 513), (1, 2047), (1, 2048), (1, 2049), (3, 171), (3, 683))
PATTERNS = ('all', 'none', 'third', 'last', 'edges')
EDGES = (63, 64, 511, 512, 2047, 2048)


def _keep(B, K, pattern):
    """(mask [B, K] bool on the device, count [B] int32: one past the last kept entry of every image)"""
    n = B * K
    i = np.arange(n)
    m = {'all': np.ones(n, bool), 'none': np.zeros(n, bool), 'third': i % 3 == 0, 'last': i == n - 1,
         'edges': np.isin(i, [e for e in EDGES if e < n])}[pattern].reshape(B, K)
    count = np.where(m.any(1), K - np.argmax(m[:, ::-1], 1), 0).astype(np.int32)
    return torch.from_numpy(m).to(DEV), torch.from_numpy(count).to(DEV)


def _gen(B, K, pattern):
    return torch.Generator(device=DEV).manual_seed(1000 * B + K + 7 * PATTERNS.index(pattern))


def _eq(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _features(B, K, pattern, C):
    """features [B, K, F] (one level, one anchor a cell), classes [B, K] with the dropped entries at -1 and C in turn, the mask
    and count"""
    g = _gen(B, K, pattern)
    x = torch.randn(B, K, F, device=DEV, generator=g)
    y = torch.randint(0, C, (B, K), device=DEV, generator=g)
    keep, count = _keep(B, K, pattern)
    out = torch.where(torch.arange(B * K, device=DEV).reshape(B, K) % 2 == 0, -1, C)
    return x, y, torch.where(keep, y, out), keep, count


@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('B,K', SHAPES)
def test_feature_ood_add(B, K, pattern):
    from ood_object_detection_amd.ood_features import FeatureOOD
    C = 3
    x, y, sparse_y, keep, count = _features(B, K, pattern, C)
    sparse, dense = FeatureOOD(F, C, 1, device=DEV), FeatureOOD(F, C, 1, device=DEV)
    sparse.add(x, sparse_y, count=count)
    if keep.any():
        dense.add(x[keep][None], y[keep][None])
    torch.cuda.synchronize()
    assert int(sparse.n_c.sum()) == int(keep.sum())
    for name in ('n_c', 's_c', 'S'):
        assert _eq(getattr(sparse, name), getattr(dense, name)), name


@pytest.mark.parametrize('sample_every', (1, 3))
@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('B,K', SHAPES)
def test_feature_knn_add(B, K, pattern, sample_every):
    from ood_object_detection_amd.ood_features import KNNFeatureOOD
    C = 3
    x, y, sparse_y, keep, count = _features(B, K, pattern, C)
    sparse, dense = (KNNFeatureOOD(F, 1, 2100, num_classes=C, sample_every=sample_every, device=DEV) for _ in range(2))
    sparse.add(x, sparse_y, count=count)
    if keep.any():
        dense.add(x[keep][None], y[keep][None])
    torch.cuda.synchronize()
    n = int(keep.sum())
    assert sparse._counts() == dense._counts() == [-(-n // sample_every), n, 0]
    size = sparse._counts()[0]
    for name in ('rows', 'norms', 'classes'):
        assert _eq(getattr(sparse, name)[:size], getattr(dense, name)[:size]), name
    if size:
        kept_y = y[keep][::sample_every]
        assert torch.equal(sparse.classes[:size].long(), kept_y)


@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('B,K', SHAPES)
def test_logit_ood_add(B, K, pattern):
    from ood_object_detection_amd.ood_logits import LogitOOD
    C = 5
    g = _gen(B, K, pattern)
    keep, count = _keep(B, K, pattern)
    z = torch.rand(B, K, C, device=DEV, generator=g) * 2 - 1                       # max z < 1 ...
    top = torch.randint(0, C, (B, K), device=DEV, generator=g)
    z = z + 4.0 * keep[..., None] * torch.nn.functional.one_hot(top, C)             # ... but >= 3 in the kept rows
    sparse, dense = LogitOOD(C, device=DEV), LogitOOD(C, device=DEV)
    sparse.add(z, count=count, min_max_logit=2.0)
    if keep.any():
        dense.add(z[keep][None])
    torch.cuda.synchronize()
    assert int(sparse.n_c.sum()) == int(keep.sum())
    for name in ('n_c', 'P_c', 'a_c', 'b_c'):
        assert _eq(getattr(sparse, name), getattr(dense, name)), name


@pytest.mark.parametrize('start', (0, 100))
@pytest.mark.parametrize('pattern', PATTERNS)
@pytest.mark.parametrize('B,K', SHAPES)
def test_ood_eval_append(B, K, pattern, start):
    from ood_object_detection_amd.ood import OODEvaluator
    g = _gen(B, K, pattern)
    keep, count = _keep(B, K, pattern)
    scores = torch.randn(B, K, device=DEV, generator=g)
    det = torch.where(keep, 0.75, 0.25)
    before = torch.randn(start, device=DEV, generator=g)
    ev = OODEvaluator(2300, 8, DEV)
    if start:
        ev.add(before, ood=False)
    ev.add_detections(scores, count, ood=False, det_scores=det, min_score=0.5)
    torch.cuda.synchronize()
    n = int(keep.sum())
    assert ev._state.tolist() == [start + n, 0, 0, 0]
    assert _eq(ev._bufs[0][:start + n], torch.cat([before, torch.masked_select(scores, keep)]))
