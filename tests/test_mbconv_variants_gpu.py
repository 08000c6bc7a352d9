"""Every fused-MBConv kernel variant the d0 ... d5 backbones run (tests/_mbconv_cases.py; coverage is asserted on the host by
test_mbconv_variants_host.py) against the float64 reference of tests/_mbconv_ref.py, per output element.  y and the SE pool
partials sit inside larger allocations between sentinel guards and start as NaN: a write past an edge tile, or an element never
written, shows.  Stride-2 cases run under both padding conventions, one case per (dtype, form) with nine images - a second
group of eight in the (B + 7) / 8 * 8 grids - against the same image run alone.

Worst measured error / bound per (dtype, form) is printed when the module's last test has run (-s); DESIGN.md records it."""
import collections

import pytest
import torch

pytestmark = pytest.mark.gpu

import _mbconv_cases as mc
import _mbconv_ref as mr

DEV = 'cuda:0'
SENTINEL = -12352.0                           # exact in bf16 and float32
IDS = ['%03d-%s' % (i, mc.case_id(c)) for i, c in enumerate(mc.CASES)]
WORST = collections.defaultdict(float)        # (dtype, form) -> worst element error / bound seen in this session
WORST_POOL = collections.defaultdict(float)


@pytest.fixture(scope='module', autouse=True)
def report_worst_ratios():
    """after the module's last test: the worst element and pool error / bound per (dtype, form) of whatever ran (shown with -s)"""
    yield
    for key in sorted(WORST):
        print('\n%-14s %-5s worst element error / bound %.3f, worst pool error / bound %.3f' %
              (mc.DTYPE_NAME[key[0]], mc.FORM_NAME[key[1]], WORST[key], WORST_POOL[key]), end='')
    print()


def _lib():
    from ood_object_detection_amd import _lib
    return _lib.load()


def _store(t, dtype):
    """float32 values -> the device tensor the kernels read (bf16, or float32-typed two-term storage)"""
    from ood_object_detection_amd import pairfmt
    t = t.contiguous()
    return (t if dtype == 0 else t.to(torch.bfloat16) if dtype == 1 else pairfmt.encode(t)).to(DEV)


def _guarded(n, guard, dtype):
    """-> (whole allocation, view of the n payload elements): [guard sentinels | n NaNs | guard sentinels]"""
    buf = torch.full((guard + n + guard,), SENTINEL, dtype=dtype, device=DEV)
    buf[guard:guard + n] = float('nan')
    return buf, buf[guard:guard + n]


def _guards_intact(buf, n, guard):
    return bool((buf[:guard] == SENTINEL).all()) and bool((buf[guard + n:] == SENTINEL).all())


def _run(case, d, pad_flag=0):
    """one launch -> (y as float32 NCHW on the CPU, pool partials [B, parts, mid] on the CPU, raw y storage on the CPU)"""
    import _hip
    from ood_object_detection_amd import pairfmt
    lib = _lib()
    dtype, gated, Cin, mid, H, W, k, s = case[:8]
    B = d['B']
    Ho, Wo = mc.same_out(H, s), mc.same_out(W, s)
    plan = mc.case_plan(lib, case)
    nt = plan['parts']
    assert nt > 0, plan
    guard = (Wo * mid + 63) // 64 * 64                     # >= one output row of elements; keeps y 16-byte aligned
    ny, npart = B * Ho * Wo * mid, B * nt * mid
    ybuf, y = _guarded(ny, guard, torch.bfloat16 if dtype == 1 else torch.float32)
    pbuf, part = _guarded(npart, guard, torch.float32)
    xd, w1d = _store(d['x'], dtype), _store(d['w1'], dtype)
    dv = [t.contiguous().to(DEV) for t in (d['s1'], d['t1'], d['wd'].permute(2, 3, 0, 1).reshape(k * k, mid), d['s2'], d['t2'])]
    st = _hip.stream(DEV)
    if gated:
        gd = d['gate'].contiguous().to(DEV)
        rc = lib.effdet_mbconv_expand_dw_gated(st, dtype | pad_flag, xd.data_ptr(), gd.data_ptr(), y.data_ptr(), w1d.data_ptr(),
                                               *[t.data_ptr() for t in dv], part.data_ptr(), B, H, W, Cin, mid, k, s)
    else:
        rc = lib.effdet_mbconv_expand_dw(st, dtype | pad_flag, xd.data_ptr(), y.data_ptr(), w1d.data_ptr(),
                                         *[t.data_ptr() for t in dv], part.data_ptr(), B, H, W, Cin, mid, k, s)
    assert rc == 0, (rc, case)
    torch.cuda.synchronize()
    assert lib.effdet_device_error(0) == 0, case
    assert _guards_intact(ybuf, ny, guard), ('y: a guard element was overwritten', case)
    assert _guards_intact(pbuf, npart, guard), ('pool partials: a guard element was overwritten', case)
    raw = y.cpu().reshape(B, Ho, Wo, mid)
    val = pairfmt.decode(raw) if dtype == 2 else raw.float()
    return val.permute(0, 3, 1, 2), part.cpu().reshape(B, nt, mid), raw


def _where(case, plan, idx):
    """'(b, y, x, c) = ...' of an NCHW index, and whether it lies in the last strip / band / tile of the plan"""
    b, c, y, x = idx
    tags = []
    if plan['form'] in (mc.ROLL, mc.WIDE):
        tags += ['last strip'] if x >= (plan['nstrips'] - 1) * plan['TWo'] else []
    if plan['form'] in (mc.ROLL, mc.WIDE, mc.DEEP):
        tags += ['last band'] if y >= (plan['nbands'] - 1) * plan['band_rows'] else []
    if plan['form'] == mc.FRONT:
        tags += ['last tile column'] if x >= (plan['tiles_x'] - 1) * plan['TW'] else []
        tags += ['last tile row'] if y >= (plan['tiles_y'] - 1) * plan['TH'] else []
    return '(b, y, x, c) = (%d, %d, %d, %d), %s' % (b, y, x, c, ', '.join(tags) if tags else 'interior')


def _check(case, d, got, part, ref, amp, what):
    plan = mc.case_plan(_lib(), case)
    key = (case[0], plan['form'])
    assert not bool(torch.isnan(got).any()), ('y: %d elements were never written' % int(torch.isnan(got).sum()), what, case[8],
                                              _where(case, plan, mr.worst(torch.isnan(got).double(), torch.ones_like(ref))[1]))
    assert not bool(torch.isnan(part).any()), ('pool partials: %d elements were never written' % int(torch.isnan(part).sum()), what, case[8])
    ratio, idx = mr.worst((got.double() - ref).abs(), mr.bound(case, ref, amp))
    Ho, Wo = ref.shape[2], ref.shape[3]
    pool = mr.pool_ok(case, part.double().sum(1) / (Ho * Wo), ref, amp)
    print('%s %s: element error / bound %.3f at %s; pool %.3f' % (mc.case_id(case), what, ratio, _where(case, plan, idx), pool))
    WORST[key] = max(WORST[key], ratio)
    WORST_POOL[key] = max(WORST_POOL[key], pool)
    assert ratio < 1.0, ('element error / bound %.3f' % ratio, what, 'class %r' % (case[8],), _where(case, plan, idx),
                         'got %r, reference %r' % (float(got[idx]), float(ref[idx])))
    assert pool < 1.0, ('pool error / bound %.3f' % pool, what, 'class %r' % (case[8],))


@pytest.mark.parametrize('case', mc.CASES, ids=IDS)
def test_variant(case):
    """one launch per padding convention (TF-SAME; stride 2: symmetric too) against the float64 reference, element by element"""
    lib = _lib()
    assert mc.case_class(lib, case) == case[8]                # the kernel this case is in the table for is the one that runs
    d = mr.make_inputs(case, mc.B)
    e = None
    for pad, flag in (('same', 0), ('', mc.PAD)) if case[7] == 2 else (('same', 0),):
        ref, amp, e = mr.reference(case, d, pad, e)
        got, part, _ = _run(case, d, flag)
        _check(case, d, got, part, ref, amp, 'TF-SAME' if pad else 'symmetric padding')
        if case[0] != 2 and pad:
            # the project's own pool check, as the existing kernel-level tests call it
            from test_kernels_gpu import _check_pool_against_oracle
            _check_pool_against_oracle(part, ref.shape[2], ref.shape[3], ref.float(), e.float(), d['wd'], d['s2'], case[6], case[7],
                                       mr.TORCH_DTYPE[case[0]])


def _one_per_dtype_form(pred):
    out = {}
    for c in mc.CASES:
        if pred(c):
            out.setdefault((c[0], c[8][2]), c)
    return [out[k] for k in sorted(out)]


STRIDE1 = _one_per_dtype_form(lambda c: c[7] == 1 and c[4] % 2 == 1)
NINE = _one_per_dtype_form(lambda c: 'odd H and odd W' in c[9])


@pytest.mark.parametrize('case', STRIDE1, ids=[mc.case_id(c) for c in STRIDE1])
def test_stride1_paddings_agree(case):
    """at stride 1 both conventions pad (k - 1) / 2 on every side: the two runs are bit-equal, y and pool partials"""
    d = mr.make_inputs(case, mc.B)
    _, p0, y0 = _run(case, d, 0)
    _, p1, y1 = _run(case, d, mc.PAD)
    assert torch.equal(y0.view(torch.int16 if case[0] == 1 else torch.int32), y1.view(torch.int16 if case[0] == 1 else torch.int32))
    assert torch.equal(p0.view(torch.int32), p1.view(torch.int32))


def test_one_case_per_dtype_and_form():
    forms = sorted(mc.CLASS_COUNTS)
    assert sorted((c[0], c[8][2]) for c in STRIDE1) == forms and sorted((c[0], c[8][2]) for c in NINE) == forms


@pytest.mark.parametrize('case', NINE, ids=[mc.case_id(c) for c in NINE])
def test_ninth_image(case):
    """B = 9: image 8 is the only image of the second group of eight (roll / wide / deep grids) or the ninth grid row (front).  It is
    correct against the reference and bit-equal, y and pool partials, to the same image run alone (geometry never depends on B)"""
    d9 = mr.make_inputs(case, 9)
    d1 = dict(d9, B=1, x=d9['x'][8:9], gate=None if d9['gate'] is None else d9['gate'][8:9])
    ref, amp, _ = mr.reference(case, d1)
    got9, part9, raw9 = _run(case, d9)
    _check(case, d1, got9[8:9], part9[8:9], ref, amp, 'image 8 of 9')
    assert not bool(torch.isnan(got9).any()) and not bool(torch.isnan(part9).any())
    got1, part1, raw1 = _run(case, d1)
    it = torch.int16 if case[0] == 1 else torch.int32
    assert torch.equal(raw9[8:9].view(it), raw1.view(it)), ('image 8 of 9 differs from the image run alone', case[8])
    assert torch.equal(part9[8:9].view(torch.int32), part1.view(torch.int32)), ('pool partials of image 8 of 9 differ', case[8])
