"""Host-side checks of the vMF hyperspherical OOD head (ood_vmf.VMFHead / VMFFeatureOOD, csrc/vmf.hip): the Bessel restatement of
tests/_vmf_ref.py against mpmath, its analytic gradients against torch autograd in float64, the ordered prototype update against the
literal per-sample loop, and the C ABI with every refusal that needs no GPU."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _vmf_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('effdet_vmf_workspace_bytes', 'effdet_vmf_partition', 'effdet_vmf_update', 'effdet_vmf_loss', 'effdet_vmf_score',
         'effdet_vmf_gather')
REL = 2.0 ** -30            # of max(1, |log Z|) and of A: 2^-24, the float32 logits these values feed, with a margin of 64


@pytest.mark.parametrize('d', [2, 3, 16, 64, 255, 256])
def test_bessel_restatement_against_mpmath(d):
    mp = pytest.importorskip('mpmath')
    mp.mp.dps = 50
    nu = mp.mpf(d) / 2 - 1
    for kappa in (2.0 ** -7, 1.0, 10.0, 100.0, 1000.0, 8192.0):
        k = mp.mpf(kappa)
        i0, i1 = mp.besseli(nu, k), mp.besseli(nu + 1, k)
        assert i0 > 0                                            # (scipy's scaled ive underflows to 0 at nu = 127, kappa = 0.01: not used)
        want_z = nu * mp.log(k) - (mp.mpf(d) / 2) * mp.log(2 * mp.pi) - mp.log(i0)
        want_a = i1 / i0
        got_z, got_a = R.log_z(d, kappa)
        ez = float(abs(mp.mpf(got_z) - want_z) / max(mp.mpf(1), abs(want_z)))
        ea = float(abs(mp.mpf(got_a) - want_a) / want_a)
        print('d %3d kappa %9.4f: log Z %.6f (error %.1e), A %.6e (error %.1e), %d terms' % (d, kappa, got_z, ez, got_a, ea, R.bessel.terms))
        assert ez <= REL and ea <= REL, (d, kappa, ez, ea)
        assert R.bessel.terms <= 1024


def test_partition_table_and_clamp():
    theta = np.array([-100.0, 100.0, np.nan, R.THETA_LO, R.THETA_HI, math.log(10.0)], np.float32)
    p = R.partition(theta, 64)
    assert list(p['clamped']) == [True, True, True, False, False, False]
    assert p['kappa'].dtype == np.float32 and np.allclose(p['kappa'], [2.0 ** -7, 8192, 2.0 ** -7, 2.0 ** -7, 8192, 10.0], rtol=1e-6)
    assert np.array_equal(p['logz32'], p['logz'].astype(np.float32))
    # d = 3 has the closed form I_{1/2}(x) = sqrt(2 / (pi x)) sinh x:  Z_3 = kappa / (4 pi sinh kappa),  A = coth kappa - 1 / kappa
    for kappa in (0.5, 3.0, 40.0):
        lz, a = R.log_z(3, kappa)
        assert abs(lz - math.log(kappa / (4 * math.pi * math.sinh(kappa)))) <= 1e-13 * max(1.0, abs(lz))
        assert abs(a - (1 / math.tanh(kappa) - 1 / kappa)) <= 1e-13


class _LogZ(torch.autograd.Function):
    """log Z_d(kappa) entered through the restated table: its value at the table's kappa, its derivative -A_d(kappa)"""
    @staticmethod
    def forward(ctx, kappa, logz, ratio):
        ctx.save_for_backward(ratio)
        return logz.clone()

    @staticmethod
    def backward(ctx, g):
        return -g * ctx.saved_tensors[0], None, None


@pytest.mark.parametrize('B,P,d,A,C,n', [(2, 12, 16, 3, 7, 30), (1, 9, 2, 1, 1, 5), (2, 10, 65, 2, 5, 17), (2, 6, 4, 9, 4, 40)])
def test_gradients_against_autograd(B, P, d, A, C, n):
    U, labels = R.inputs(B, P, d, A, C, n)
    proto, valid = R.update(U, labels, A, np.zeros((C, d), np.float32), np.zeros(C, bool))
    theta = np.log(np.random.RandomState(C).uniform(2.0, 40.0, C)).astype(np.float32)
    part = R.partition(theta, d)
    ref = R.forward(U, labels, A, proto, valid, part)
    assert ref['m'] > 0 and ref['m'] == n - int((~valid[labels.reshape(-1)[(labels.reshape(-1) >= 0) & (labels.reshape(-1) < C)]]).sum())
    Ut = torch.from_numpy(U.astype(np.float64)).requires_grad_()
    th = torch.from_numpy(np.log(part['kappa'].astype(np.float64))).requires_grad_()
    kappa = th.exp()
    logz = _LogZ.apply(kappa, torch.from_numpy(part['logz32'].astype(np.float64)), torch.from_numpy(part['ratio']))
    cell = torch.from_numpy(ref['idx'] // A)
    r = F.normalize(Ut.reshape(B * P, d)[cell], dim=1, eps=R.EPS)
    l = logz[None] + kappa[None] * (r @ torch.from_numpy(proto.astype(np.float64)).t())
    keep = torch.from_numpy(np.nonzero(valid)[0])
    y = torch.from_numpy(np.searchsorted(np.nonzero(valid)[0], ref['y']))
    lv = l[:, keep]
    loss = (torch.logsumexp(lv, 1) - lv[torch.arange(len(y)), y]).mean()
    gU, gth = torch.autograd.grad(loss, [Ut, th])
    assert abs(float(loss.detach()) - ref['loss']) <= 1e-12 * max(1.0, abs(ref['loss']))
    for name, got, want in (('dU', ref['dU'], gU.numpy()), ('dtheta', ref['dtheta'], gth.numpy())):
        err, scale = np.abs(got - want).max(), np.abs(want).max()
        print('%s: max |value| %.3e, error %.1e' % (name, scale, err))
        assert err <= 1e-11 * max(scale, 1e-300), (name, err, scale)
    # the float32 form stays near it; a clamped class has no gradient
    f32 = R.forward(U, labels, A, proto, valid, part, np.float32)
    for k, (e32, bd) in R.bounds(ref, f32).items():
        scale = np.abs(np.asarray(ref[{'loss': 'loss_i', 'mean_dot': 'dot_y'}.get(k, k)])).max()
        assert e32 <= 1e-4 * scale and bd >= 4 * e32, (k, e32, scale)
    cl = R.forward(U, labels, A, proto, valid, dict(part, clamped=np.arange(C) == 0))
    assert cl['dtheta'][0] == 0 and np.array_equal(cl['dtheta'][1:], ref['dtheta'][1:])


@pytest.mark.parametrize('limit', [None, 1, 3])
def test_ordered_update_equals_the_per_sample_loop(limit):
    U, labels = R.inputs(2, 40, 16, 3, 6, 90)
    U[1, 5, 3], labels[1, 15] = np.nan, 2                        # a counted anchor on a non-finite row: skipped
    labels[0, :3] = (6, -1, 99)                                  # labels outside [0, C)
    p0, v0 = np.zeros((6, 16), np.float32), np.zeros(6, bool)
    a = R.update(U, labels, 3, p0, v0, 0.9, limit)
    b = R.update_literal(U, labels, 3, p0, v0, 0.9, limit)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1]) and a[1].any()
    assert np.allclose(np.linalg.norm(a[0][a[1]], axis=1), 1.0, atol=1e-6) and not a[0][~a[1]].any()
    # the rows of one call applied in two calls give the same bits (the update of image 0, then that of image 1)
    if limit is None:
        h = R.update(U[:1], labels[:1], 3, p0, v0, 0.9)
        h = R.update(U[1:], labels[1:], 3, h[0], h[1], 0.9)
        assert np.array_equal(h[0].view(np.uint32), a[0].view(np.uint32))
    f = R.flags(U, labels, 3, 6)
    assert f[120 + 15] == -2 and set(np.nonzero(f == -2)[0] // 3) == {40 + 5}          # only the anchors of that cell


def test_entry_points_declared_bound_and_exported():
    from ood_object_detection_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'effdet_hip.h')).read()
    lib = _lib.load()
    for name in NAMES:
        m = re.search(r'\b%s\s*\(([^;]*)\);' % name, header)
        assert m, name
        assert len(_lib.SIGNATURES[name][1]) == m.group(1).count(',') + 1, name
        assert hasattr(lib, name), name
    assert sorted(n for n in _lib.SIGNATURES if n.startswith('effdet_vmf_')) == sorted(NAMES)
    mk = open(os.path.join(_lib.CSRC, 'Makefile')).read()
    assert 'build/vmf.o' in mk and re.search(r'EXTRA_vmf\s*=\s*-ffp-contract=off', mk)
    assert re.search(r'build/vmf\.o:\s*feature_rows\.h compact\.h wave_rows\.h', mk)
    src = open(os.path.join(_lib.CSRC, 'vmf.hip')).read()
    # row addressing, label reading, compaction, tile constants, the carve and the in-wave primitives are the shared headers'
    assert '#include "feature_rows.h"' in src and '#include "wave_rows.h"' in src
    assert 'fo_count_kernel<VmRows>' in src and 'fo_base_kernel<VmRows>' in src and 'fo_write_index_kernel<VmRows>' in src
    assert 'fo_class(' in src and 'fo_select(' in src and 'FoCarve' in src and 'wr_argmax<' in src and 'wr_for_classes(' in src
    assert not re.search(r'void \w+_(count|base)_kernel\(', src) and 'fo_block_excl_scan(unsigned' not in src
    assert not re.search(r'DEV int \w+_min\(', src) and not re.search(r'\bCp? <= 128\b', src) and not re.search(r'int \w+_NONE\b', src)
    assert not re.search(r'atomic\w*\(', src) and 'hipMalloc' not in src and 'Synchronize' not in src


def test_argument_refusals_before_any_launch():
    """every call below must return -22 from pure host code: nothing is launched"""
    from ood_object_detection_amd import _lib
    lib = _lib.load()
    q = lib.effdet_vmf_workspace_bytes
    assert 0 < q(1, 1, 2) <= q(100, 90, 64) < q(1 << 27, 90, 64) and q(100, 90, 64) < q(100, 1024, 256)
    for bad in ((0, 90, 64), (-1, 90, 64), ((1 << 27) + 1, 90, 64), (100, 0, 64), (100, 1025, 64), (100, 90, 1), (100, 90, 257)):
        assert q(*bad) == -22, bad
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)                                 # any non-null address: nothing is dereferenced on the host
    big = 1 << 40

    def part(theta=p, C=90, d=64, outs=(p,) * 5):
        return lib.effdet_vmf_partition(None, theta, C, d, *outs)

    def update(U=p, B=1, P=10, A=9, d=64, cls=p, dt=1, pitch=90, stride=1, C=90, alpha=0.95, lim=0, pr=p, va=p, ws=p, nb=big):
        return lib.effdet_vmf_update(None, U, B, P, A, d, cls, dt, pitch, stride, 0, C, alpha, lim, pr, va, ws, nb)

    def loss(U=p, B=1, P=10, A=9, d=64, cls=p, dt=1, pitch=90, stride=1, C=90, ins=(p,) * 6, outs=(p,) * 4, ws=p, nb=big):
        return lib.effdet_vmf_loss(None, U, B, P, A, d, cls, dt, pitch, stride, 0, C, *ins, *outs, ws, nb)

    def score(U=p, B=1, P=10, A=9, d=64, K=5, C=90, ins=(p,) * 4, outs=(p,) * 3, ws=p, nb=big):
        return lib.effdet_vmf_score(None, U, B, P, A, d, K, None, None, 0, 0, C, *ins, *outs, None, ws, nb)

    assert part(theta=None) == -22 and part(C=0) == -22 and part(C=1025) == -22 and part(d=1) == -22 and part(d=257) == -22
    for k in range(5):
        assert part(outs=tuple(None if i == k else p for i in range(5))) == -22
    need = q(90, 90, 64)
    for fn in (update, loss):
        assert fn(U=None) == -22 and fn(B=0) == -22 and fn(P=0) == -22 and fn(A=0) == -22 and fn(d=1) == -22 and fn(d=257) == -22
        assert fn(cls=None) == -22 and fn(dt=3) == -22 and fn(dt=-1) == -22 and fn(pitch=-1) == -22 and fn(stride=-1) == -22
        assert fn(C=0) == -22 and fn(C=1025) == -22 and fn(ws=None) == -22 and fn(nb=need - 1) == -22
        assert fn(B=1 << 14, P=1 << 14) == -22 and fn(P=1 << 27, A=2) == -22
    for kw in (dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=float('nan')), dict(lim=-1), dict(pr=None), dict(va=None)):
        assert update(**kw) == -22, kw
    for k in range(6):
        assert loss(ins=tuple(None if i == k else p for i in range(6))) == -22
    for k in range(4):
        assert loss(outs=tuple(None if i == k else p for i in range(4))) == -22
    assert score(U=None) == -22 and score(B=0) == -22 and score(P=0) == -22 and score(A=0) == -22 and score(K=0) == -22
    assert score(d=1) == -22 and score(d=257) == -22 and score(C=0) == -22 and score(C=1025) == -22 and score(ws=None) == -22
    assert score(nb=q(5, 90, 64) - 1) == -22 and score(B=1 << 14, K=1 << 14) == -22
    for k in range(4):
        assert score(ins=tuple(None if i == k else p for i in range(4))) == -22
    for k in range(3):
        assert score(outs=tuple(None if i == k else p for i in range(3))) == -22
    arr = lambda v, t: (t * len(v))(*v)
    tab = lambda **kw: (kw.get('n', 1), arr([p], ctypes.c_void_p), arr([kw.get('cells', 4)], ctypes.c_longlong), arr([256], ctypes.c_longlong),
                        arr([64], ctypes.c_longlong), arr([kw.get('ch', 1)], ctypes.c_longlong))

    def gather(dtype=0, F=64, A=9, B=1, K=5, out=p, **kw):
        return lib.effdet_vmf_gather(None, dtype, *tab(**kw), F, A, B, K, None, None, 0, out)
    assert gather(dtype=2) == -22 and gather(F=63) == -22 and gather(A=0) == -22 and gather(B=0) == -22 and gather(K=0) == -22
    assert gather(out=None) == -22 and gather(n=0) == -22 and gather(n=9) == -22 and gather(cells=0) == -22 and gather(ch=2) == -22


def test_constructor_refusals_and_the_scorer_list():
    from ood_object_detection_amd.effdet.bench import _feature_scorers
    from ood_object_detection_amd.ood_vmf import VMFFeatureOOD, VMFHead, partition
    head = VMFHead(64, 5, 9, dim=16)                              # (constructors allocate on the CPU: no device is needed here)
    assert tuple(head.weight1.shape) == (64, 64) and tuple(head.weight2.shape) == (16, 64) and tuple(head.log_kappa.shape) == (5,)
    assert abs(float(head.log_kappa[0]) - math.log(10.0)) < 1e-6
    sd = head.state_dict()
    assert tuple(sd['prototypes'].shape) == (5, 16) and sd['valid'].dtype == torch.int32 and not sd['valid'].any()
    assert sorted(n for n, _ in head.named_parameters()) == ['log_kappa', 'weight1', 'weight2']
    s = VMFFeatureOOD(head)
    assert s.KEYS == R.KEYS and s.WANTS_CLASS_TOWER is True and _feature_scorers([s]) == (s,)
    with pytest.raises(ValueError, match='vmf'):
        _feature_scorers([s, VMFFeatureOOD(head)])
    for kw in (dict(num_features=63), dict(num_classes=0), dict(num_classes=1025), dict(num_anchors=0), dict(dim=1), dict(dim=257),
               dict(hidden=0), dict(kappa_init=0.0), dict(kappa_init=1e5), dict(ema=-0.1), dict(ema=1.1), dict(ema_rows_per_class=0)):
        with pytest.raises(ValueError):
            VMFHead(**dict(dict(num_features=64, num_classes=5, num_anchors=9), **kw))
    with pytest.raises(ValueError, match='VMFHead'):
        VMFFeatureOOD(object())
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        head.loss(torch.zeros(1, 4, 16), torch.zeros(1, 36, dtype=torch.int64))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        head([torch.zeros(1, 64, 2, 2)], torch.zeros(1, 36, dtype=torch.int64))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        partition(head.log_kappa.detach(), 16)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        s.score([torch.zeros(1, 64, 2, 2)], torch.zeros(1, 2, dtype=torch.int64))
    with pytest.raises(ValueError):
        head.loss(torch.zeros(1, 4, 15), torch.zeros(1, 36, dtype=torch.int64))
    with pytest.raises(ValueError):
        head.embed(torch.zeros(1, 4, 63))
