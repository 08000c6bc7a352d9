"""Host-side checks of the meta-phase inner update (no GPU): episode.plan_inner_update against the literal loop of infer.py:661-678
over the MetaHead's parameter names, the C entry points are declared, bound and exported, and the limits query answers on the host."""
import ctypes
import os
import re

import pytest
import torch

import _inner_update_ref as iref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = {'effdet_inner_update': 10, 'effdet_inner_update_backward': 14, 'effdet_inner_update_max_tensors': 0,
                'effdet_inner_update_max_step_sizes': 0, 'effdet_inner_update_workspace_doubles': 2}


def test_inner_update_entry_points_declared_bound_and_exported():
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


def test_limits_are_answered_on_the_host():
    from ood_object_detection_amd import _lib
    lib = _lib.load()
    assert lib.effdet_inner_update_max_tensors() >= 24
    assert lib.effdet_inner_update_max_step_sizes() >= 8
    lls = lambda v: (ctypes.c_longlong * len(v))(*v)
    one = lib.effdet_inner_update_workspace_doubles(1, lls([1]))
    assert one > 0
    assert lib.effdet_inner_update_workspace_doubles(2, lls([1, 82944])) > one                   # grows with the workgroups
    assert lib.effdet_inner_update_workspace_doubles(1, lls([0])) == -1                           # empty tensor
    assert lib.effdet_inner_update_workspace_doubles(1, lls([2 ** 30 + 1])) == -1
    assert lib.effdet_inner_update_workspace_doubles(lib.effdet_inner_update_max_tensors() + 1, lls([1] * 64)) == -1


def test_bad_arguments_are_einval_before_any_launch():
    """null pointers, counts and step-size indices outside the limits: -22 from the host checks (nothing is launched, so no GPU)"""
    from ood_object_detection_amd import _lib
    lib = _lib.load()
    P = lambda v: (ctypes.c_void_p * len(v))(*v)
    lls = lambda v: (ctypes.c_longlong * len(v))(*v)
    ints = lambda v: (ctypes.c_int * len(v))(*v)
    fl = lambda v: (ctypes.c_float * len(v))(*v)
    ok = dict(n=1, p=P([64]), g=P([128]), o=P([192]), count=lls([4]), idx=ints([0]), n_lr=1, lrp=P([None]), lrv=fl([0.1]))

    def fwd(**kw):
        a = dict(ok, **kw)
        return lib.effdet_inner_update(None, a['n'], a['p'], a['g'], a['o'], a['count'], a['idx'], a['n_lr'], a['lrp'], a['lrv'])

    def bwd(**kw):
        a = dict(ok, **kw)
        return lib.effdet_inner_update_backward(None, a['n'], a['p'], a['g'], a['o'], a['count'], a['idx'], a['n_lr'], a['lrp'], a['lrv'],
                                                a.get('ws'), a.get('ws_doubles', 0), 0, a.get('dlr'))

    for call in (fwd, bwd):
        assert call(n=0) == -22
        assert call(n=lib.effdet_inner_update_max_tensors() + 1) == -22
        assert call(p=P([None])) == -22
        assert call(g=P([None])) == -22
        assert call(p=None) == -22
        assert call(count=lls([0])) == -22
        assert call(count=lls([2 ** 30 + 1])) == -22
        assert call(idx=ints([1])) == -22
        assert call(idx=ints([-1])) == -22
        assert call(n_lr=0) == -22
        assert call(n_lr=lib.effdet_inner_update_max_step_sizes() + 1) == -22
        assert call(lrp=None) == -22
    assert fwd(o=P([None])) == -22
    assert bwd(dlr=8, ws=None) == -22                        # a reduction is wanted but there is no workspace
    assert bwd(dlr=8, ws=256, ws_doubles=1) == -22           # ... or one that is too small
    assert bwd(dlr=8, ws=260, ws_doubles=64) == -22          # ... or not 8-byte aligned


@pytest.mark.parametrize('only_final,separate_head', [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize('add_head', [False, True])
@pytest.mark.parametrize('layers', [3, 4])
def test_plan_equals_the_literal_loop(layers, add_head, only_final, separate_head):
    from ood_object_detection_amd.episode import plan_inner_update
    names = iref.meta_head_names(layers, 5, add_head)
    assert len(names) == 3 * layers + 3 + 2 * 5 * layers + (2 if add_head else 0)
    n_lr = 1 if only_final else layers + 2                                  # infer.py:243-250
    want = iref.literal_plan(names, n_lr, only_final, separate_head)
    got = plan_inner_update(names, n_lr, only_final, separate_head)
    assert got == want
    assert all(k is None or 0 <= k < n_lr for k in got)
    by = dict(zip(names, got))
    assert all(by[n] is None for n in names if n.startswith('bn_'))
    if only_final:
        assert by['conv_dw0'] is None and by['predict_dw'] is None
        moved = [n for n in names if by[n] is not None]
        assert moved == (['predict_pw_sep', 'predict_pb_sep'] if separate_head and add_head else [] if separate_head else
                         ['predict_pw', 'predict_pb'] + (['predict_pw_sep', 'predict_pb_sep'] if add_head else []))
    else:
        assert [by['conv_dw%d' % l] for l in range(layers)] == list(range(layers)) and by['predict_dw'] == layers
        assert by['predict_pw'] == (None if separate_head else layers + 1)
        if add_head:
            assert by['predict_pb_sep'] == layers + 1


@pytest.mark.parametrize('only_final', [False, True])
@pytest.mark.parametrize('layers', [3, 4])
def test_plan_raises_where_the_literal_loop_raises(layers, only_final):
    """every list length from 1 to layers + 2: the literal loop either indexes (then the plans agree, negative indices included) or
    raises IndexError (then plan_inner_update raises ValueError naming the parameter)"""
    from ood_object_detection_amd.episode import plan_inner_update
    names = iref.meta_head_names(layers, 5, True)
    raised = 0
    for n_lr in range(1, layers + 3):
        try:
            want = iref.literal_plan(names, n_lr, only_final, False)
        except IndexError:
            raised += 1
            with pytest.raises(ValueError, match='conv_dw|predict_dw'):
                plan_inner_update(names, n_lr, only_final, False)
            continue
        assert plan_inner_update(names, n_lr, only_final, False) == want
    assert raised == (0 if only_final else layers - 1)          # without only_final: conv_dw<l> needs l + 1 entries, predict_dw two
    with pytest.raises(ValueError):
        plan_inner_update(names, 0)
    with pytest.raises(IndexError):
        iref.literal_plan(['conv_dw'], 3)
    with pytest.raises(ValueError, match="'conv_dw'"):
        plan_inner_update(['conv_dw'], 3)                        # no character at position 7
    with pytest.raises(ValueError):
        iref.literal_plan(['conv_dwx'], 3)
    with pytest.raises(ValueError, match="'conv_dwx'"):
        plan_inner_update(['conv_dwx'], 3)                       # not a digit


def test_cpu_tensors_raise():
    from ood_object_detection_amd import episode
    p, g = torch.zeros(4), torch.ones(4)
    with pytest.raises(RuntimeError, match='GPU'):
        episode.inner_update([('conv_dw0', p)], [g], [0.1, 0.1])
    with pytest.raises(ValueError):
        episode.inner_update([('conv_dw0', p)], [g, g], [0.1, 0.1])                 # one gradient too many
    # nothing to update: every entry passes through as the same object, with or without a GPU
    bn = torch.zeros(4)
    assert episode.inner_update([('bn_w00', bn), ('conv_dw0', p)], [g, None], [0.1, 0.1])[0] is bn
