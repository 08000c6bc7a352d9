"""Detection-level OOD metrics without a GPU: the float64 restatement (tests/_ood_eval_ref.py) against its brute-force form and
against scikit-learn, the pure-host queries of csrc/ood_eval.hip, and the argument checks of ood.detection_metrics / OODEvaluator."""
import numpy as np
import pytest
import torch

import _ood_eval_ref as R


def _cases():
    rs = np.random.RandomState(3)
    yield 'ties', np.round(rs.normal(0.3, 1, 57) * 2) / 2, np.round(rs.normal(0, 1, 41) * 2) / 2
    yield 'continuous', rs.normal(0.5, 1, 64), rs.normal(0, 1, 33)
    yield 'all equal', np.full(9, 0.25), np.full(5, 0.25)
    yield 'separated', rs.uniform(1, 2, 7), rs.uniform(-2, -1, 11)
    yield 'reversed', rs.uniform(-2, -1, 7), rs.uniform(1, 2, 11)
    yield 'zeros', np.array([-0.0, 0.0, 1.0, -1.0]), np.array([0.0, -0.0, 2.0])
    yield 'single', np.array([0.5]), np.array([0.5])
    yield 'specials', np.array([np.inf, -np.inf, 1e-45, -1e-45, 3.4e38, 0.0]), np.array([np.inf, -3.4e38, 1e-45, 0.0, -np.inf])


@pytest.mark.parametrize('level', [0.95, 1.0, 0.5, 1e-9])
def test_restatement_equals_brute_force(level):
    for name, pos, neg in _cases():
        a, b = R.metrics(pos, neg, level), R.metrics_brute(pos, neg, level)
        for k in R.INT_KEYS + ('threshold', 'groups_in', 'groups_out', 'auroc', 'tpr', 'fpr_at_tpr', 'aupr_in', 'aupr_out'):
            assert a[k] == b[k], (name, level, k, a[k], b[k])


def test_rank_at_level():
    assert R.rank_at_level(20, 0.95) == 19 and R.rank_at_level(20, 1.0) == 20 and R.rank_at_level(20, 1e-9) == 1
    assert R.rank_at_level(3, 2 / 3) == 2 and R.rank_at_level(1, 0.95) == 1
    for P in (1, 7, 100, 4097, 1 << 20):
        for level in (0.95, 0.5, 1 / 3, 0.999999, 1.0):
            k = R.rank_at_level(P, level)
            assert float(k) / float(P) >= level and (k == 1 or float(k - 1) / float(P) < level)


def test_nan_is_refused():
    with pytest.raises(ValueError):
        R.metrics(np.array([0.0, np.nan]), np.array([1.0]))


def test_restatement_equals_sklearn():
    skm = pytest.importorskip('sklearn.metrics')
    for name, pos, neg in _cases():
        if name == 'specials':
            continue                    # scikit-learn refuses infinite scores
        pos, neg = R.canonical(pos), R.canonical(neg)
        y = np.concatenate([np.ones(pos.size), np.zeros(neg.size)])
        s = np.concatenate([pos, neg]).astype(np.float64)
        for level in (0.95, 0.5, 1.0):
            m = R.metrics(pos, neg, level)
            assert abs(m['auroc'] - skm.roc_auc_score(y, s)) <= 1e-12, name
            assert abs(m['aupr_in'] - skm.average_precision_score(y, s)) <= 1e-12, name
            assert abs(m['aupr_out'] - skm.average_precision_score(1 - y, -s)) <= 1e-12, name
            fpr, tpr, _ = skm.roc_curve(y, s, drop_intermediate=False)
            i = int(np.argmax(tpr >= level))
            assert m['fp'] == int(round(fpr[i] * neg.size)) and m['tp'] == int(round(tpr[i] * pos.size)), (name, level)
            assert abs(m['fpr_at_tpr'] - fpr[i]) <= 1e-12 and abs(m['tpr'] - tpr[i]) <= 1e-12


def test_host_queries():
    from ood_object_detection_amd import _lib
    lib = _lib.load()
    T = lib.effdet_ood_eval_sort_tile()
    assert T > 0 and T % 64 == 0
    small, large = lib.effdet_ood_eval_workspace_bytes(1000, 1000), lib.effdet_ood_eval_workspace_bytes(1 << 20, 1000)
    assert 0 < small < large
    assert large - small >= 2 * 4 * ((1 << 20) - 1000)              # two key buffers a side
    assert lib.effdet_ood_eval_workspace_bytes(1000, 1 << 20) > small
    for bad in ((0, 10), (10, 0), ((1 << 27) + 1, 10)):
        assert lib.effdet_ood_eval_workspace_bytes(*bad) == -22
    assert lib.effdet_ood_eval_workspace_bytes(1 << 27, 1 << 27) > 0
    o0, o1 = (lib.effdet_ood_eval_sorted_offset(1000, 2000, s) for s in (0, 1))
    assert 0 < o0 and o0 + 4000 <= o1 and o1 + 8000 <= lib.effdet_ood_eval_workspace_bytes(1000, 2000)


def test_python_api_refuses_cpu_tensors_and_bad_levels():
    from ood_object_detection_amd import ood
    x = torch.zeros(4)
    with pytest.raises(RuntimeError):
        ood.detection_metrics(x, x)
    with pytest.raises(RuntimeError):
        ood.OODEvaluator(8, 8).add(x, False)
    with pytest.raises(RuntimeError):
        ood.OODEvaluator(8, 8).add_detections(x.reshape(1, 4), None, True)
    with pytest.raises(RuntimeError):
        ood.OODEvaluator(8, 8, device='cpu')
    for level in (0.0, -0.5, 1.5, float('nan')):
        with pytest.raises(ValueError):
            ood.detection_metrics(x, x, recall_level=level)
        with pytest.raises(ValueError):
            ood.OODEvaluator(8, 8).evaluate(recall_level=level)
    with pytest.raises(ValueError):
        ood.OODEvaluator(0, 8)
