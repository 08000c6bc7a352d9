"""Host-side checks of the episode stage (no GPU): the entry points are declared, bound and exported; kept_per_level agrees with
what torch.quantile keeps; CPU tensors are refused; and the lean float64 form of tests/_episode_ref.py - the yardstick of the GPU
tests where the literal n x n form cannot run - equals the literal form."""
import ctypes
import os
import re

import pytest
import torch

import _episode_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {'effdet_episode_select': 8, 'effdet_episode_feed': 21, 'effdet_episode_cluster_workspace_floats': 3,
                'effdet_episode_cluster': 25}


def test_episode_entry_points_declared_bound_and_exported():
    from ood_object_detection_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'effdet_hip.h')).read()
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    import torch  # noqa: F401  (share torch's HIP runtime, see _lib.load)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in ENTRY_POINTS.items():
        assert re.search(r'\b(int|long long)\s+%s\s*\(' % name, header), name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
        assert hasattr(lib, name), name
    lib.effdet_episode_cluster_workspace_floats.restype = ctypes.c_longlong
    assert lib.effdet_episode_cluster_workspace_floats(6300, 256, 25) > 6300          # pure host arithmetic
    assert lib.effdet_episode_cluster_workspace_floats(6300, 256, 65) == -1           # m * d > 16384
    assert lib.effdet_episode_cluster_workspace_floats(6301, 256, 25) == -1           # n % m != 0


@pytest.mark.parametrize('side,n,kept', [(8, 576, 72), (16, 2304, 288), (32, 9216, 1152), (64, 36864, 4608), (5, 225, 28), (6, 324, 41),
                                         (4, 144, 144), (2, 36, 36), (1, 9, 9)])
def test_kept_per_level_matches_torch_quantile(side, n, kept):
    from ood_object_detection_amd.episode import kept_per_level
    assert kept_per_level(side, side) == kept
    res_conf = ref.tie_free_confs(side, 3, n)
    assert ref.tie_free(res_conf)
    mask = ref.quantile_mask(res_conf, side)
    assert mask.sum(1).tolist() == [kept] * 3


def test_cpu_tensors_raise():
    from ood_object_detection_amd import episode
    with pytest.raises(RuntimeError):
        episode.select_anchors([torch.zeros(2, 9, 8, 8)])
    with pytest.raises(RuntimeError):
        episode.cluster(torch.zeros(10, 8), torch.zeros(10), 2, 1.0, 0.0)
    with pytest.raises(RuntimeError):
        episode.target_from_selection(torch.zeros(10, 8), torch.zeros(10), {}, 1.0, 0.0)

    class Net:
        anch_enc, lev_enc, cell_enc = torch.zeros(9, 8), torch.zeros(5, 6), torch.zeros(80, 14)
    with pytest.raises(RuntimeError):
        episode.projection_feed([torch.zeros(2, 64, 8, 8)], [torch.zeros(2, 9, 8, 8)], [torch.zeros(2, 72, dtype=torch.int32)], Net())


@pytest.mark.parametrize('num,rows,d', [(25, 252, 256), (5, 1692, 128), (7, 100, 64)])
@pytest.mark.parametrize('valid_threshold', [None, 0.05])
def test_lean_form_equals_literal_form(num, rows, d, valid_threshold):
    x, confs = ref.clustered_rows(1000 + num, num, rows, d)
    x, confs = x.double(), confs.double()
    for sim_target in ('max', 'avg'):
        lit = ref.cluster_literal(x, confs, 3., 3., num, valid_threshold, sim_target)
        lean = ref.cluster_lean(x, confs, 3., 3., num, valid_threshold, sim_target)
        assert 0 < int(lit['valid'].sum())
        for k in ('proto0', 'valid', 'proto') + (('nearest',) if sim_target == 'max' else ()):
            assert torch.equal(lit[k], lean[k]), k
        for k in ('soft_thresh', 'avg_init0', 'avg_init', 'target_clust', 'sim', 'target'):
            assert float((lit[k] - lean[k]).abs().max()) <= 1e-12, k
    # the scores the lean form decides on (and tests/_episode_ref.py::decision_gaps measures) are the literal ones
    n = num * rows
    if n <= 7000:
        e = torch.nn.functional.normalize(x, p=2)
        s = lit['soft_thresh']
        ws = ((s[:, None] * s[None, :]) * (e @ e.t())).reshape(num, rows, n)
        assert float((ws.mean(2) - lean['score0']).abs().max()) <= 1e-12
