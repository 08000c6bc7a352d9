"""Host side of the grouped optimizer (optim.GroupedOptimizer, csrc/group_optim.hip): the layout planner, the torch reference
driver against itself (which defines the tolerance yardstick E32 of tests/test_group_optim_gpu.py), and the argument checks of
the new entry points.  No GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _group_optim_ref as R

SIZES = [1, 1, 15, 16, 17, 63, 64, 65, 100003]        # the first stands for a 0-d tensor (one element)


def _check_layout(numels, group_of, domain_of, lay):
    from ood_object_detection_amd import optim
    n = len(numels)
    assert sorted(lay['order']) == list(range(n))
    spans = sorted((lay['offsets'][i], lay['offsets'][i] + lay['padded'][i]) for i in range(n))
    for i in range(n):
        assert lay['offsets'][i] % 16 == 0                          # 64 bytes
        assert lay['padded'][i] % 16 == 0 and numels[i] <= lay['padded'][i] < numels[i] + 16
    assert spans[0][0] == 0 and spans[-1][1] == lay['total']
    assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))      # no overlap, no hole
    n_dom = max([d for d in domain_of if d is not None and d >= 0], default=-1) + 1
    assert len(lay['domain_ranges']) == n_dom
    for d, (lo, hi) in enumerate(lay['domain_ranges']):             # each domain: one contiguous range holding exactly its tensors
        inside = [i for i in range(n) if lo <= lay['offsets'][i] < hi]
        assert inside == [i for i in range(n) if domain_of[i] == d]
        assert sum(lay['padded'][i] for i in inside) == hi - lo
    # parameter order is kept inside a domain and among the tensors in no domain
    key = [(domain_of[i] if domain_of[i] is not None and domain_of[i] >= 0 else n_dom) for i in lay['order']]
    assert key == sorted(key)
    for d in set(key):
        part = [i for i, k in zip(lay['order'], key) if k == d]
        assert part == sorted(part)
    # the device tables: pieces tile every segment, never straddle one, and a domain is one range of pieces
    pieces, seg_group, dom_ranges = lay['pieces'], lay['seg_group'], lay['dom_ranges']
    assert pieces.dtype == np.int32 and pieces.shape[1] == 4 and dom_ranges.shape == (n_dom + 1, 4)
    pos = 0
    for off4, n4, seg, _ in pieces.tolist():
        i = lay['order'][seg]
        assert off4 * 4 == pos and 0 < n4 * 4 <= optim.PIECE_FLOATS
        assert lay['offsets'][i] <= pos and pos + n4 * 4 <= lay['offsets'][i] + lay['padded'][i]
        pos += n4 * 4
    assert pos == lay['total']
    assert seg_group.tolist() == [(-1 if group_of[i] is None else group_of[i]) for i in lay['order']]
    for d in range(n_dom + 1):
        pb, pe, sb, se = dom_ranges[d].tolist()
        assert [lay['order'][s] for s in range(sb, se)] == [i for i in lay['order'] if (domain_of[i] if domain_of[i] is not None and domain_of[i] >= 0 else n_dom) == d]
        assert sorted(set(pieces[pb:pe, 2].tolist())) == list(range(sb, se))
    assert lay['n_norm_pieces'] == (dom_ranges[n_dom][0] if n_dom else 0)
    assert dom_ranges[n_dom][1] == len(pieces) and dom_ranges[n_dom][3] == n


@pytest.mark.parametrize('case', ['interleaved', 'one', 'no_domain', 'norm_only_last', 'empty_domain'])
def test_plan_layout(case):
    from ood_object_detection_amd import optim
    n = len(SIZES)
    if case == 'interleaved':
        group_of = [i % 3 for i in range(n)]
        domain_of = [1, 0, -1, 1, 0, None, 0, 1, 0]
        group_of[7] = -1                                            # in a domain and in no group
    elif case == 'one':
        group_of, domain_of = [0] * n, [0] * n
    elif case == 'no_domain':
        group_of, domain_of = [i % 2 for i in range(n)], [-1] * n
    elif case == 'norm_only_last':
        group_of, domain_of = [0] * (n - 1) + [None], [None] * (n - 1) + [0]
    else:
        group_of, domain_of = [0] * n, [2 if i % 2 else 0 for i in range(n)]     # domain 1 has no tensor
    lay = optim.plan_layout(SIZES, group_of, domain_of)
    _check_layout(SIZES, group_of, domain_of, lay)
    # the same plan whatever else happens: a pure function
    again = optim.plan_layout(list(SIZES), list(group_of), list(domain_of))
    assert again['offsets'] == lay['offsets'] and np.array_equal(again['pieces'], lay['pieces'])


def test_plan_layout_rejects():
    from ood_object_detection_amd import optim
    with pytest.raises(ValueError):
        optim.plan_layout([4, 4], [0, -1], [-1, -1])                # a tensor in no group and in no domain
    with pytest.raises(ValueError):
        optim.plan_layout([4, 0], [0, 0], [0, 0])                   # empty tensor
    with pytest.raises(ValueError):
        optim.plan_layout([4, 4], [0], [0, 0])
    with pytest.raises(ValueError):
        optim.plan_layout([], [], [])
    assert optim.membership(4, [[0, 2], [3]]) == [0, -1, 0, 1]
    with pytest.raises(ValueError):
        optim.membership(4, [[0, 2], [2]])                          # in two groups
    with pytest.raises(ValueError):
        optim.membership(4, [[0, 0]])                               # twice in one
    with pytest.raises(ValueError):
        optim.membership(4, [[4]])


@pytest.mark.parametrize('optim', ['adam', 'sgd'])
def test_reference_driver_and_e32(optim):
    """The driver on the GPU test's scenario: float64 against float32 gives E32; the scenario does what it claims (exactly one
    domain clips in step 2, step counts diverge, the absent tensor keeps its bits)."""
    ref, e = R.scenario_pair(optim)
    print('E32 %s: parameters %.3e, state1 %.3e, state2 %.3e' % (optim, e['params'], e['state1'], e['state2']))
    assert 0.0 < e['params'] < 1e-5 and 0.0 < e['state1'] < 1e-5 and e['state2'] < 1e-5
    assert len(ref) == R.STEPS
    assert ref[1]['coefs'][0] == 1.0 and ref[1]['coefs'][1] < 1.0
    assert all(c == 1.0 for k in (0, 2) for c in ref[k]['coefs'])
    p0, _ = R.scenario_data()
    for snap in ref:
        for i in (R.NEVER, R.NORM_ONLY):
            assert np.array_equal(snap['params'][i], p0[i].astype(np.float64)) and snap['steps'][i] == 0
    last = ref[-1]['steps']
    if optim == 'adam':
        assert last[0] == 6 and last[3] == 5 and last[4] == 5       # absent once: one count behind
    else:
        assert last[0] == 1 and last[3] == 1
        assert ref[0]['steps'][3] == 0 and ref[1]['steps'][3] == 1   # SGD's first-buffer rule applies at step 2
    # group 1 sits at lr 0 until the edit
    g1 = R.scenario_groups()[1]['params']
    for i in g1:
        assert np.array_equal(ref[2]['params'][i], p0[i].astype(np.float64))
        assert not np.array_equal(ref[3]['params'][i], p0[i].astype(np.float64))
    # the driver is deterministic
    again = R.scenario_reference(optim, torch.float64)
    assert all(np.array_equal(a, b) for s, t in zip(ref, again) for a, b in zip(s['params'], t['params']))


def test_group_entry_points_refuse_bad_arguments():
    """-22 for null pointers and zero sizes, before anything is launched (no GPU here)."""
    from ood_object_detection_amd import _lib, optim
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = _lib.load()
    assert lib.effdet_group_piece_floats() == optim.PIECE_FLOATS
    buf = (ctypes.c_int * 64)()
    ok = ctypes.addressof(buf)
    #            stream kind p   g   s1  s2  n   pieces n_p n_np seg_group n_seg dom n_dom dyn n_groups step const partial norms
    good = [None, 0, ok, ok, ok, ok, 16, ok, 1, 0, ok, 1, ok, 0, ok, 1, ok, ok, ok, ok]
    for pos in (2, 3, 4, 5, 7, 10, 12, 14, 16, 17, 18, 19):         # each pointer null in turn
        args = list(good)
        args[pos] = None
        assert lib.effdet_group_step(*args) == -22, pos
    for pos, bad in ((1, 2), (6, 0), (6, 24), (8, 0), (9, 2), (11, 0), (13, -1), (15, 0)):
        args = list(good)
        args[pos] = bad
        assert lib.effdet_group_step(*args) == -22, (pos, bad)
    #             stream g   n   pieces n_p n_np seg_group n_seg dom n_dom dyn n_groups partial norms
    goodn = [None, ok, 16, ok, 1, 1, ok, 1, ok, 1, ok, 0, ok, ok]
    for pos in (1, 3, 6, 8, 10, 12, 13):
        args = list(goodn)
        args[pos] = None
        assert lib.effdet_group_norms(*args) == -22, pos
    for pos, bad in ((2, 0), (4, 0), (7, 0), (9, 0)):
        args = list(goodn)
        args[pos] = bad
        assert lib.effdet_group_norms(*args) == -22, (pos, bad)


def test_grouped_optimizer_has_no_cpu_fallback():
    from ood_object_detection_amd import optim
    p = torch.nn.Parameter(torch.zeros(5))
    before = p.data_ptr()
    with pytest.raises(RuntimeError):
        optim.GroupedOptimizer([{'params': [p]}])
    assert p.data_ptr() == before and p.grad is None
    with pytest.raises(NotImplementedError):
        optim.GroupedOptimizer([{'params': [p]}], amsgrad=True)
    with pytest.raises(NotImplementedError):
        optim.GroupedOptimizer([{'params': [p]}], optim='sgd', momentum=0.9, dampening=0.1)
    with pytest.raises(ValueError):
        optim.GroupedOptimizer([{'params': [p]}, {'params': [p]}])


def test_script_param_groups():
    """the lists of pretrain.py:181-185 and infer.py:259-274 / :803-804"""
    from ood_object_detection_amd import optim

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.backbone, self.fpn, self.box_net = torch.nn.Linear(2, 2), torch.nn.Linear(2, 2), torch.nn.Linear(2, 2)
            self.class_net = torch.nn.Module()
            for n in ('conv', 'predict_pw', 'predict_pb', 'predict_pw_sep', 'predict_pb_sep'):
                setattr(self.class_net, n, torch.nn.Parameter(torch.zeros(2)))
    m, proj, lrs = Net(), torch.nn.Linear(3, 3), [torch.nn.Parameter(torch.tensor(0.01))]
    ids = lambda ps: [id(p) for p in ps]
    groups, domains = optim.script_param_groups(m, meta_lr=2e-3)
    assert [g['lr'] for g in groups] == [0., 2e-3, 2e-3]
    assert ids(groups[0]['params']) == ids(m.fpn.parameters()) and ids(groups[2]['params']) == ids(m.box_net.parameters())
    assert len(domains) == 1 and ids(domains[0]['params']) == ids(m.parameters()) and domains[0]['max_norm'] == 10.0
    groups, _ = optim.script_param_groups(m, meta_lr=2e-3, train_bb=True)
    assert [g['lr'] for g in groups] == [2e-3] * 4 and ids(groups[0]['params']) == ids(m.backbone.parameters())
    groups, domains = optim.script_param_groups(m, proj_net=proj, learnable_lr=lrs, meta_lr=1e-4, max_norm=3.0)
    assert [g['lr'] for g in groups] == [1e-4, 1e-4, 1e-4, 0.]
    assert ids(groups[0]['params']) == ids([m.class_net.predict_pw, m.class_net.predict_pb])
    assert len(groups[1]['params']) == 3 and ids(groups[3]['params']) == ids(lrs)
    assert [d['max_norm'] for d in domains] == [3.0, 3.0]
    assert ids(domains[0]['params']) == ids(proj.parameters()) and ids(domains[1]['params']) == ids(m.parameters())
    groups, _ = optim.script_param_groups(m, proj_net=proj, learnable_lr=lrs, meta_lr=1e-4, separate_head=True)
    assert [g['lr'] for g in groups] == [1e-4, 0., 0., 0.]
    assert ids(groups[0]['params']) == ids([m.class_net.predict_pw_sep, m.class_net.predict_pb_sep])
