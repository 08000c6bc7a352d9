"""Case table of tests/test_train_forms_{host,gpu}.py: one small problem per kernel class of the training GEMMs and depthwise
entries of csrc/train_net.hip that the d0 ... d5 training step runs, plus the edge shapes of every class.  No GPU code here:
the plan of a call is asked of the host-only queries effdet_train_gemm_nt_plan_describe / _gemm_tn_plan_describe /
_dwconv_plan_describe, which are answered by the launchers' own decision code.

A call (and the head of a case) is a tuple:
    ('nt', entry, M, K, N, akind, ckind, pk, lv, operands, a_rows, align)     entry: gemm_nt / gemm_nt_fused / gemm_nt_relu /
                                                                              gemm_nt_mask / gemm_nt_levels
    ('tn', entry, M, N, K, ykind, pk, lv, x_rows, align)                      entry: gemm_tn / gemm_tn_scaled / gemm_tn_levels
    ('dw', which, B, H, W, C, k, s, pad, flag)                                which: fwd (flag: A and the pool partial rows are
                                                                              written) / bwd_dx (flag: Z) / bwd_dw (flag: cmajor)
kind of a row map: DENSE, STRIDED (rows_per_image, img_stride, ld = pk) or LEVELS (the level-packed map of the *_levels entries:
lv = (B, ((h, w), ...)), pk = (0, img_stride, ld)); at most one side of a call is not dense.  operands: the EFFDET_NT_HAS_* bits;
a_rows / x_rows: rows per image of the SE gate (0: none); align: address mod 16 of A, W, C, bias, R, C2, a_scale, mask (nt) or of
dY, X, x_scale (tn); pad: 0 TF-SAME, 1 symmetric.  A case is call + (cls, edges): the class it is meant to reach and the names
of the edges (NT_EDGES / TN_EDGES / DW_EDGES) it is in the table for.

A kernel class is the entry point's kernel plus everything that selects code:
    nt: ('nt', VEC, KS, FAST, EPI, floats per store, operands, akind, ckind)
    tn: ('tn', body, VY, VX, DENSE, SCALED, ykind, slices)        slices: 0 S == 1, 1 S > 1, 2 S > 1 with empty trailing slices
    dw: ('dw', 'fwd', k, s, pad at stride 2, flag, blocks_per_image > 1, strips_x > 1, channel groups > 1)
        ('dw', 'bwd_dx', 4-pixel stride-1 kernel, k, s, pad at stride 2, flag, workgroups > 1)
        ('dw', 'bwd_dw', k, s, pad at stride 2, flag, seg == 32, segs_per_chunk > 4, chunks > 1, channel groups > 1)
CLASS_COUNTS and CASES are generated (the block between CASES-BEGIN and CASES-END) by tools/make_train_cases.py, which sweeps
swept_calls(), searches the cheapest problem of every class and of every edge and rewrites that block in place
(tests/test_train_forms_host.py fails when the table and the sweep disagree)."""
import ctypes

from _mbconv_cases import MAX_ELEMS, MODELS, SIZES, same_out  # noqa: F401  (re-exported: the limits of the two tables are the same)

PAD = 1 << 24                                 # EFFDET_PAD_SYMMETRIC
NT_INTS, TN_INTS, DW_INTS = 7, 11, 13
OVER_LIMIT_FACTOR = 3                         # a class that no problem within MAX_ELEMS reaches (OVER_LIMIT) may take this much more
NT_FIELDS = ('VEC', 'KS', 'FAST', 'EPI', 'vec_out', 'grid', 'kchunk')
TN_FIELDS = ('body', 'VY', 'VX', 'DENSE', 'SCALED', 'S', 'rows_per_slice', 'empty', 'gx', 'gy', 'gz')
DW_FIELDS = ('Ho', 'Wo', 'pad_t', 'pad_l', 'cgroups', 'blocks_per_image', 'strips_x', 'dx_s1', 'dx_blocks', 'seg', 'segs_x',
             'segs_per_chunk', 'chunks')
BIAS, RES, C2, A_SCALE, ACC, MASK = 1, 2, 4, 8, 16, 32       # EFFDET_NT_HAS_* / EFFDET_NT_ACCUMULATE
OPERAND_NAME = {BIAS: 'bias', RES: 'R', C2: 'C2', A_SCALE: 'gate', ACC: 'acc', MASK: 'mask'}
DENSE, STRIDED, LEVELS = 0, 1, 2
KIND_NAME = {DENSE: 'dense', STRIDED: 'strided', LEVELS: 'levels'}
EPI = {'gemm_nt': 0, 'gemm_nt_fused': 0, 'gemm_nt_levels': 0, 'gemm_nt_relu': 1, 'gemm_nt_mask': 2}
DW_WHICH = {'fwd': 0, 'bwd_dx': 1, 'bwd_dw': 2}
A16_NT, A16_TN = (0,) * 8, (0,) * 3

# batch sizes of the sweep: 2, 3, 4 and 8 images are what the suite's training steps run (tests/test_train_gpu.py,
# test_not_cls_train_gpu.py, test_pad0_gpu.py, test_dropin_gpu.py), 8 is also the default of tools/pretrain_bench.py
BATCHES = (2, 3, 4, 8)
# class counts of the sweep: 90 (COCO, the models' own) and the small ones the suite builds models with
NUM_CLASSES = (90, 20, 12, 7, 6, 5, 3, 1)
NUM_ANCHORS = 9
# ProjectionNet (effdet/aux_nets.py): widths and row counts the suite and the tools run, both depths
PROJ_WIDTHS = (64, 128, 512)
PROJ_ROWS = (63, 300, 6300)


def _ints(n):
    return (ctypes.c_int * n)()


def nt_plan(lib, call):
    _, entry, M, K, N, akind, ckind, pk, lv, ops, a_rows, align = call[:12]
    a = (int(akind == LEVELS),) + (tuple(pk) if akind != DENSE else (0, 0, 0))
    c = (int(ckind == LEVELS),) + (tuple(pk) if ckind != DENSE else (0, 0, 0))
    out = _ints(NT_INTS)
    n = lib.effdet_train_gemm_nt_plan_describe(M, K, N, a[0], a[1], a[2], a[3], c[0], c[1], c[2], c[3], ops, a_rows, EPI[entry],
                                               (ctypes.c_int * 8)(*align), out, NT_INTS)
    return dict(zip(NT_FIELDS, out)) if n == NT_INTS else None


def tn_plan(lib, call):
    _, entry, M, N, K, ykind, pk, lv, x_rows, align = call[:10]
    y = (int(ykind == LEVELS),) + (tuple(pk) if ykind != DENSE else (0, 0, 0))
    out = _ints(TN_INTS)
    n = lib.effdet_train_gemm_tn_plan_describe(M, N, K, y[0], y[1], y[2], y[3], 0, 0, 0, 0, x_rows, (ctypes.c_int * 3)(*align), out, TN_INTS)
    return dict(zip(TN_FIELDS, out)) if n == TN_INTS else None


def dw_plan(lib, call):
    _, which, B, H, W, C, k, s, pad, flag = call[:10]
    out = _ints(DW_INTS)
    n = lib.effdet_train_dwconv_plan_describe(DW_WHICH[which], H, W, C, k | (PAD if pad else 0), s, B, out, DW_INTS)
    return dict(zip(DW_FIELDS, out)) if n == DW_INTS else None


def plan(lib, call):
    """the library's plan of a call as a dict (None: the query refuses the call)"""
    return {'nt': nt_plan, 'tn': tn_plan, 'dw': dw_plan}[call[0]](lib, call)


def klass(p, call):
    """the kernel class of a call whose plan is p"""
    if call[0] == 'nt':
        return ('nt', p['VEC'], p['KS'], p['FAST'], p['EPI'], p['vec_out'], call[9], call[5], call[6])
    if call[0] == 'tn':
        return ('tn', p['body'], p['VY'], p['VX'], p['DENSE'], p['SCALED'], call[5], 0 if p['S'] == 1 else 2 if p['empty'] else 1)
    _, which, B, H, W, C, k, s, pad, flag = call[:10]
    pad2 = pad if s == 2 else 0
    if which == 'fwd':
        return ('dw', which, k, s, pad2, flag, int(p['blocks_per_image'] > 1), int(p['strips_x'] > 1), int(p['cgroups'] > 1))
    if which == 'bwd_dx':
        return ('dw', which, p['dx_s1'], k, s, pad2, flag, int(p['dx_blocks'] > 1))
    return ('dw', which, k, s, pad2, flag, int(p['seg'] == 32 and p['segs_x'] > 1), int(p['segs_per_chunk'] > 4), int(p['chunks'] > 1),
            int(p['cgroups'] > 1))


def call_class(lib, call):
    p = plan(lib, call)
    return None if p is None else klass(p, call)


def family(cls):
    """the row of the class table a class is counted in"""
    if cls[0] == 'nt':
        return 'gemm_nt<%d,%d,%s>%s' % (cls[1], cls[2], 'fast' if cls[3] else 'general', ('', ' relu', ' mask')[cls[4]])
    if cls[0] == 'tn':
        return ('gemm_tn<%d,%s>' % (cls[2], 'vx' if cls[3] else 'scalar x'), 'gemm_tn_v<%s%s,%d>' % ('dense' if cls[4] else 'mapped',
                ',scaled' if cls[5] else '', cls[2]), 'gemm_tn_w<%s,%d>' % ('dense' if cls[4] else 'mapped', cls[2]))[cls[1]]
    if cls[1] == 'bwd_dx':
        return 'dw_bwd_dx%s' % ('_s1<%d>' % cls[3] if cls[2] else ' general k%d' % cls[3])
    return 'dw_%s<%d,%d>' % (cls[1], cls[2], cls[3])


def elems(call):
    """the largest operand or output of a call, in elements"""
    if call[0] == 'nt':
        _, entry, M, K, N, akind, ckind, pk, lv, ops, a_rows, align = call[:12]
        a = M * K if akind == DENSE else packed_floats(call)
        c = M * N if ckind == DENSE else packed_floats(call)
        return max(a, c, N * K)
    if call[0] == 'tn':
        _, entry, M, N, K, ykind, pk, lv, x_rows, align = call[:10]
        return max(M * N if ykind == DENSE else packed_floats(call), M * K, N * (K + 1))
    _, which, B, H, W, C, k, s, pad, flag = call[:10]
    return B * H * W * C


def packed_floats(call):
    """floats of the image-major tensor behind the non-dense side of a GEMM call"""
    M = call[2]
    pk, lv = (call[7], call[8]) if call[0] == 'nt' else (call[6], call[7])
    if lv is not None:
        return lv[0] * pk[1]
    return (M + pk[0] - 1) // pk[0] * pk[1]


def levels_rows(lv):
    return lv[0] * sum(h * w for h, w in lv[1])


def case_id(case):
    cls = case[-2]
    if case[0] == 'nt':
        _, entry, M, K, N, akind, ckind, pk, lv, ops, a_rows, align = case[:12]
        names = '+'.join(v for b, v in sorted(OPERAND_NAME.items()) if ops & b) or 'plain'
        s = '%s-v%dks%d%s-st%d-%s-a_%s-c_%s-M%d-K%d-N%d' % (entry, cls[1], cls[2], 'f' if cls[3] else 'g', cls[5], names, KIND_NAME[akind],
                                                             KIND_NAME[ckind], M, K, N)
    elif case[0] == 'tn':
        _, entry, M, N, K, ykind, pk, lv, x_rows, align = case[:10]
        s = '%s-b%dvy%dvx%d%s%s-y_%s-sl%d-M%d-N%d-K%d' % (entry, cls[1], cls[2], cls[3], 'd' if cls[4] else 'm', 's' if cls[5] else '',
                                                         KIND_NAME[ykind], cls[7], M, N, K)
    else:
        _, which, B, H, W, C, k, s_, pad, flag = case[:10]
        s = 'dw_%s-k%ds%d%s%s-B%d-%dx%dx%d' % (which, k, s_, '-sym' if pad else '', '-flag' if flag else '', B, H, W, C)
    if any(case[11 if case[0] == 'nt' else 9]) if case[0] != 'dw' else False:
        s += '-al' + ''.join('%x' % v for v in case[11 if case[0] == 'nt' else 9])
    return s + ('-e%d' % len(case[-1]) if case[-1] else '')


# ---- the sweep ------------------------------------------------------------------------------------------------
def _nt(entry, M, K, N, ops=0, a_rows=0, akind=DENSE, ckind=DENSE, pk=(0, 0, 0), lv=None, align=A16_NT):
    return ('nt', entry, M, K, N, akind, ckind, pk, lv, ops, a_rows, align)


def _tn(entry, M, N, K, x_rows=0, ykind=DENSE, pk=(0, 0, 0), lv=None, align=A16_TN):
    return ('tn', entry, M, N, K, ykind, pk, lv, x_rows, align)


def _bneval_fwd(M, K, N, silu=False, rows=0, resid=False):
    """TrainEngine._pw_bneval_fwd: the folded shift is the second row of a [3, N] buffer, so its address is 4 N mod 16"""
    ops = BIAS | (C2 if silu else 0) | (A_SCALE if rows else 0) | (RES if resid else 0)
    return _nt('gemm_nt_fused', M, K, N, ops, rows, align=(0, 0, 0, 4 * N % 16, 0, 0, 0, 0))


def _bneval_bwd(M, K, N, rows=0, resid=False, need_dx=True):
    """TrainEngine._pw_bneval_bwd of a conv with K inputs and N outputs"""
    out = [_tn('gemm_tn_scaled', M, N, K, rows) if rows else _tn('gemm_tn', M, N, K)]
    if need_dx:
        out.append(_nt('gemm_nt_fused', M, N, K, RES if resid else 0))
    return out


def backbone_blocks(model):
    from ood_object_detection_amd.backbone import efficientnet_arch
    from ood_object_detection_amd.effdet.config import get_efficientdet_config
    cfg = get_efficientdet_config(model)
    stem_c, stages = efficientnet_arch(cfg.backbone_name)
    return cfg, stem_c, stages


def backbone_calls(model, size, B):
    """every call of TrainEngine._bb_forward / _bb_backward -> (calls, [(channels, h, w) of the three feature maps])"""
    cfg, stem_c, stages = backbone_blocks(model)
    h = w = same_out(size, 2)
    calls = [_bneval_fwd(B * h * w, 32, stem_c, silu=True)] + _bneval_bwd(B * h * w, 32, stem_c, need_dx=False)
    feats = []
    for si, blocks in enumerate(stages):
        for b in blocks:
            k, s, cin, mid, cout = b['k'], b['s'], b['cin'], b['mid'], b['cout']
            ho, wo = same_out(h, s), same_out(w, s)
            Mi, Mo = B * h * w, B * ho * wo
            ir = b['type'] == 'ir'
            C = mid if ir else cin
            if ir:
                calls.append(_bneval_fwd(Mi, cin, mid, silu=True))
                calls += _bneval_bwd(Mi, cin, mid, resid=b['residual'])
            for pad in ((0, 1) if s == 2 else (0,)):             # tf_* models pad TF-SAME, the others symmetrically (timm pad_type)
                calls.append(('dw', 'fwd', B, h, w, C, k, s, pad, 1))
                calls.append(('dw', 'bwd_dx', B, h, w, C, k, s, pad, int(ir)))
                calls.append(('dw', 'bwd_dw', B, h, w, C, k, s, pad, 0))
            for resid in ((True, False) if b['residual'] else (False,)):      # a dropped path (stochastic depth) skips the shortcut
                calls.append(_bneval_fwd(Mo, C, cout, rows=ho * wo, resid=resid))
            calls += _bneval_bwd(Mo, C, cout, rows=ho * wo)
            h, w = ho, wo
        if si in (2, 4, 6):
            feats.append((stages[si][-1]['cout'], h, w))
    return calls, feats


def _pw(M, K, N, bias, need_dx=True):
    """TrainEngine._pw_fwd / _pw_bwd of a conv with K inputs and N outputs"""
    out = [_nt('gemm_nt', M, K, N, BIAS if bias else 0), _tn('gemm_tn', M, N, K)]
    if need_dx:
        out.append(_nt('gemm_nt', M, N, K))
    return out


def fpn_head_calls(model, feats, B, num_classes):
    """every call of TrainEngine._fh_forward / _fh_backward (BiFPN, class and box towers, predict layers)"""
    from ood_object_detection_amd.effdet.config import get_efficientdet_config
    from ood_object_detection_amd.effdet.config.fpn_config import get_fpn_config
    cfg = get_efficientdet_config(model)
    F, L = cfg.fpn_channels, cfg.num_levels
    nbb = len(feats)
    rbias = (not cfg.apply_resample_bn) or cfg.redundant_bias
    hw = [(h, w) for _, h, w in feats]
    calls = []
    calls += _pw(B * hw[-1][0] * hw[-1][1], feats[-1][0], F, rbias)            # fpn.resample of the first extra level
    while len(hw) < L:
        hw.append((same_out(hw[-1][0], 2), same_out(hw[-1][1], 2)))
    fc = get_fpn_config(cfg.fpn_name, min_level=cfg.min_level, max_level=cfg.max_level)
    for node in fc.nodes:                                                    # the backbone features enter the first cell through a conv
        for off in node['inputs_offsets']:
            if off < nbb and feats[off][0] != F:
                calls += _pw(B * hw[off][0] * hw[off][1], feats[off][0], F, rbias)
    pads = (0, 1)
    for (h, w) in hw:                                                        # after_combine: depthwise 3x3 + 1x1 conv, every level
        for pad in pads[:1]:                                                 # stride 1: the padding convention selects no code
            calls.append(('dw', 'fwd', B, h, w, F, 3, 1, pad, 0))
            calls.append(('dw', 'bwd_dx', B, h, w, F, 3, 1, pad, 0))
            calls.append(('dw', 'bwd_dw', B, h, w, F, 3, 1, pad, 1))
        calls += _pw(B * h * w, F, F, cfg.redundant_bias)
    lv = (B, tuple(hw))
    M = levels_rows(lv)
    P = sum(h * w for h, w in hw)
    calls += _pw(M, F, F, cfg.redundant_bias)                                # conv_rep over the packed pyramid
    for NO in (NUM_ANCHORS * num_classes, NUM_ANCHORS * 4):                  # predict: written into / read from the head tensor
        pk = (0, P * NO, NO)
        calls.append(_nt('gemm_nt_levels', M, F, NO, BIAS, ckind=LEVELS, pk=pk, lv=lv))
        calls.append(_tn('gemm_tn_levels', M, NO, F, ykind=LEVELS, pk=pk, lv=lv))
        calls.append(_nt('gemm_nt_levels', M, NO, F, akind=LEVELS, pk=pk, lv=lv))
    return calls


def projection_calls(model):
    """the gemm_nt_relu / gemm_nt_mask pair of effdet/meta_ops.py ProjLinear over ProjectionNet's layers (depth 2 and 3)"""
    from ood_object_detection_amd.effdet.config import get_efficientdet_config
    F = get_efficientdet_config(model).fpn_channels
    calls = []
    for width in PROJ_WIDTHS:
        for M in PROJ_ROWS:
            calls.append(_nt('gemm_nt_relu', M, F + 42, width))               # first layer
            calls.append(_nt('gemm_nt_relu', M, width, width))                # a middle layer (depth 3)
            for n_next in (width, width // 2):                                # d input of the layer after a ReLU
                calls.append(_nt('gemm_nt_mask', M, n_next, width, MASK))
    return calls


_SWEEP = {}


def sizes_of(model):
    from ood_object_detection_amd.effdet.config import get_efficientdet_config
    return sorted({get_efficientdet_config(model).image_size[0]} | set(SIZES))


def swept_calls(model, size, B):
    """the set of distinct calls of one training step of `model` at size x size with B images (every class count of NUM_CLASSES)"""
    key = (model, size, B)
    if key not in _SWEEP:
        calls, feats = backbone_calls(model, size, B)
        for nc in NUM_CLASSES:
            calls += fpn_head_calls(model, feats, B, nc)
        _SWEEP[key] = set(calls)
    return _SWEEP[key]


def all_swept_calls():
    out = set()
    for model in MODELS:
        out |= set(projection_calls(model))
        for size in sizes_of(model):
            for B in BATCHES:
                out |= swept_calls(model, size, B)
    return out


def used_classes(lib):
    """{class: the swept calls that have it}"""
    used = {}
    for call in all_swept_calls():
        c = call_class(lib, call)
        assert c is not None, call
        used.setdefault(c, []).append(call)
    return used


# ---- edges: (name, applies(class), holds(plan, case)) ------------------------------------------------------------
def _nt_m(p, c):
    M = c[2]
    return M > 128 and M % 32 != 0 and (p['KS'] == 4 or 0 < M % 128 <= 96)


NT_EDGES = (
    ('M % 128 and M % 32 != 0, last wave without a row', lambda k: True, _nt_m),
    ('N > 64, N % 64 != 0', lambda k: True, lambda p, c: c[4] > 64 and c[4] % 64 != 0),        # a second, ragged column block
    ('N % 16 a non-zero multiple of 4', lambda k: k[5] == 4, lambda p, c: c[4] % 16 in (4, 8, 12)),
    ('N % 16 == 2', lambda k: k[5] == 2, lambda p, c: c[4] % 16 == 2),
    ('N odd', lambda k: k[5] == 0, lambda p, c: c[4] % 2 == 1),
    ('K % 16 != 0', lambda k: True, lambda p, c: c[3] % 16 != 0),
    # without split-K a wave walks all of K: both pipeline stages run, then a lone last step with a ragged tail
    ('K > 32, K % 32 > 16', lambda k: k[2] == 1, lambda p, c: c[3] > 32 and c[3] % 32 > 16),
    ('K == 4', lambda k: k[3] == 1 and k[2] == 1, lambda p, c: c[3] == 4),
    ('split-K, K % 64 != 0', lambda k: k[2] == 4, lambda p, c: c[3] % 64 != 0),
    ('split-K, K % 64 == 0', lambda k: k[2] == 4, lambda p, c: c[3] % 64 == 0),
    ('C rows with ld > N', lambda k: k[8] != DENSE, lambda p, c: c[7][2] > c[4]),
    ('gate rows not dividing 32', lambda k: bool(k[6] & A_SCALE), lambda p, c: 32 % c[10] != 0 and c[10] % 32 != 0 and c[2] >= 2 * c[10]),
)
# edges that one problem cannot carry together go to separate cases: every combo lists what is searched jointly
NT_COMBOS = (
    ('M % 128 and M % 32 != 0, last wave without a row', 'N > 64, N % 64 != 0', 'N % 16 a non-zero multiple of 4', 'N % 16 == 2', 'N odd',
     'K % 16 != 0', 'K > 32, K % 32 > 16', 'split-K, K % 64 != 0', 'C rows with ld > N', 'gate rows not dividing 32'),
    ('K == 4',),
    ('split-K, K % 64 == 0',),
)


def _tn_m(p, c):
    return c[2] % 32 != 0 and c[2] % p['rows_per_slice'] != 0


TN_EDGES = (
    ('M % 32 != 0, M no multiple of rows_per_slice', lambda k: True, _tn_m),
    ('an empty trailing slice', lambda k: k[7] == 2, lambda p, c: p['empty'] > 0),
    ('N % 32 != 0', lambda k: k[1] != 2, lambda p, c: c[3] % 32 != 0),
    ('N % 128 != 0', lambda k: k[1] == 2, lambda p, c: c[3] % 128 != 0),
    ('K % 64 == 0', lambda k: True, lambda p, c: c[4] % 64 == 0),
    ('K % 64 == 60', lambda k: True, lambda p, c: c[4] % 64 == 60),
    ('K % 64 neither 0 nor 60', lambda k: True, lambda p, c: c[4] % 64 not in (0, 60)),
    ('gate rows not dividing 16', lambda k: bool(k[5]), lambda p, c: 16 % c[8] != 0 and c[8] % 16 != 0 and c[2] >= 2 * c[8]),
)
_TN_COMMON = ('M % 32 != 0, M no multiple of rows_per_slice', 'an empty trailing slice', 'N % 32 != 0', 'N % 128 != 0',
              'gate rows not dividing 16')
TN_COMBOS = (_TN_COMMON + ('K % 64 == 0',), _TN_COMMON + ('K % 64 == 60',), _TN_COMMON + ('K % 64 neither 0 nor 60',))

def _dw_big(k):
    # (a forward class with one strip a row has Wo <= 4: at stride 1 no map wider than 5 taps fits)
    return not (k[1] == 'fwd' and k[7] == 0 and k[3] == 1 and k[2] == 5)


DW_EDGES = (
    ('H > k and W > k', _dw_big, lambda p, c: c[3] > c[6] and c[4] > c[6]),        # every tap meets data in both directions
    ('W % 4 != 0 and Wo % 4 != 0', lambda k: True, lambda p, c: c[4] % 4 != 0 and p['Wo'] % 4 != 0),
    ('odd H and W at stride 2', lambda k: (k[3] if k[1] != 'bwd_dx' else k[4]) == 2, lambda p, c: c[3] % 2 == 1 and c[4] % 2 == 1),
    ('C > 64, C % 64 != 0', lambda k: k[1] == 'bwd_dx' or k[-1] == 1, lambda p, c: c[5] > 64 and c[5] % 64 != 0),
    ('ragged last block of an image', lambda k: k[1] == 'fwd' and k[6] == 1, lambda p, c: (p['strips_x'] * p['Ho']) % 128 != 0),
    ('Wo > 48, Wo % 32 != 0', lambda k: k[1] == 'bwd_dw' and k[6] == 1, lambda p, c: p['Wo'] > 48 and p['Wo'] % 32 != 0),
)
DW_COMBOS = (tuple(e[0] for e in DW_EDGES),)

EDGES = {'nt': NT_EDGES, 'tn': TN_EDGES, 'dw': DW_EDGES}
COMBOS = {'nt': NT_COMBOS, 'tn': TN_COMBOS, 'dw': DW_COMBOS}


def applicable(cls):
    """names of the edges that apply to a class"""
    return [e[0] for e in EDGES[cls[0]] if e[1](cls)]


def holds(name, p, case):
    return next(e[2] for e in EDGES[case[0]] if e[0] == name)(p, case)


# ---- value bound of the exact run: every operand element is an integer of magnitude 1 ... 3 ---------------------------
def exact_bound(call):
    """an upper bound of sum |products| over every partial sum of the integer reference of a call (any order)"""
    if call[0] == 'nt':
        K, ops = call[3], call[9]
        return K * 9 * (3 if ops & A_SCALE else 1) + 3 * (bool(ops & BIAS) + bool(ops & RES) + bool(ops & ACC))
    if call[0] == 'tn':
        return call[2] * 9 * (3 if call[8] else 1)
    _, which, B, H, W, C, k, s, pad, flag = call[:10]
    if which == 'fwd':
        return k * k * 9 * 3 + 3
    if which == 'bwd_dx':
        return k * k * 9
    return B * same_out(H, s) * same_out(W, s) * 9


# CASES-BEGIN
# classes per kernel that the sweep of all_swept_calls() finds (recorded in DESIGN.md; the host test recounts them)
CLASS_COUNTS = {
    'dw_bwd_dw<3,1>': 14,
    'dw_bwd_dw<3,2>': 6,
    'dw_bwd_dw<5,1>': 4,
    'dw_bwd_dw<5,2>': 8,
    'dw_bwd_dx general k3': 2,
    'dw_bwd_dx general k5': 2,
    'dw_bwd_dx_s1<3>': 3,
    'dw_bwd_dx_s1<5>': 1,
    'dw_fwd<3,1>': 10,
    'dw_fwd<3,2>': 4,
    'dw_fwd<5,1>': 3,
    'dw_fwd<5,2>': 6,
    'gemm_nt<1,1,general>': 1,
    'gemm_nt<2,1,general>': 1,
    'gemm_nt<2,1,general> relu': 1,
    'gemm_nt<2,4,general>': 1,
    'gemm_nt<4,1,fast>': 9,
    'gemm_nt<4,1,fast> mask': 1,
    'gemm_nt<4,1,fast> relu': 1,
    'gemm_nt<4,1,general>': 1,
    'gemm_nt<4,4,fast>': 6,
    'gemm_nt<4,4,fast> mask': 1,
    'gemm_nt<4,4,fast> relu': 1,
    'gemm_tn<1,vx>': 2,
    'gemm_tn_v<dense,4>': 3,
    'gemm_tn_v<dense,scaled,4>': 3,
    'gemm_tn_v<mapped,2>': 2,
    'gemm_tn_v<mapped,4>': 2,
    'gemm_tn_w<dense,4>': 3,
    'gemm_tn_w<mapped,2>': 2,
}

# classes that no problem within MAX_ELEMS reaches (their cases are the cheapest that do)
OVER_LIMIT = [
    ('dw', 'bwd_dw', 3, 2, 0, 0, 1, 1, 1, 1),
    ('dw', 'bwd_dw', 3, 2, 1, 0, 1, 1, 1, 1),
    ('dw', 'bwd_dw', 5, 2, 0, 0, 1, 1, 1, 1),
    ('dw', 'bwd_dw', 5, 2, 1, 0, 1, 1, 1, 1),
]

# fmt: off
CASES = [
    ('dw', 'bwd_dw', 1, 5, 1, 68, 3, 1, 0, 0, ('dw', 'bwd_dw', 3, 1, 0, 0, 0, 0, 1, 1), ()),
    ('dw', 'bwd_dw', 1, 5, 5, 68, 3, 1, 0, 0, ('dw', 'bwd_dw', 3, 1, 0, 0, 0, 0, 1, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'C > 64, C % 64 != 0')),
    ('dw', 'bwd_dw', 3, 683, 1, 68, 3, 1, 0, 0, ('dw', 'bwd_dw', 3, 1, 0, 0, 0, 1, 1, 1), ()),
    ('dw', 'bwd_dw', 3, 683, 5, 68, 3, 1, 0, 0, ('dw', 'bwd_dw', 3, 1, 0, 0, 0, 1, 1, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'C > 64, C % 64 != 0')),
    ('dw', 'bwd_dw', 1, 1, 129, 4, 3, 1, 0, 0, ('dw', 'bwd_dw', 3, 1, 0, 0, 1, 0, 1, 0), ()),
    ('dw', 'bwd_dw', 1, 4, 49, 4, 3, 1, 0, 0, ('dw', 'bwd_dw', 3, 1, 0, 0, 1, 0, 1, 0), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'Wo > 48, Wo % 32 != 0')),
    ('dw', 'bwd_dw', 1, 1, 129, 68, 3, 1, 0, 0, ('dw', 'bwd_dw', 3, 1, 0, 0, 1, 0, 1, 1), ()),
    ('dw', 'bwd_dw', 1, 4, 49, 68, 3, 1, 0, 0, ('dw', 'bwd_dw', 3, 1, 0, 0, 1, 0, 1, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'C > 64, C % 64 != 0', 'Wo > 48, Wo % 32 != 0')),
    ('dw', 'bwd_dw', 2, 683, 65, 4, 3, 1, 0, 0, ('dw', 'bwd_dw', 3, 1, 0, 0, 1, 1, 1, 0), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'Wo > 48, Wo % 32 != 0')),
    ('dw', 'bwd_dw', 1, 683, 65, 68, 3, 1, 0, 0, ('dw', 'bwd_dw', 3, 1, 0, 0, 1, 1, 1, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'C > 64, C % 64 != 0', 'Wo > 48, Wo % 32 != 0')),
    ('dw', 'bwd_dw', 1, 1, 1, 4, 3, 1, 0, 1, ('dw', 'bwd_dw', 3, 1, 0, 1, 0, 0, 0, 0), ()),
    ('dw', 'bwd_dw', 1, 4, 5, 4, 3, 1, 0, 1, ('dw', 'bwd_dw', 3, 1, 0, 1, 0, 0, 0, 0), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0')),
    ('dw', 'bwd_dw', 1, 1, 1, 68, 3, 1, 0, 1, ('dw', 'bwd_dw', 3, 1, 0, 1, 0, 0, 0, 1), ()),
    ('dw', 'bwd_dw', 1, 4, 5, 68, 3, 1, 0, 1, ('dw', 'bwd_dw', 3, 1, 0, 1, 0, 0, 0, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'C > 64, C % 64 != 0')),
    ('dw', 'bwd_dw', 1, 5, 1, 4, 3, 1, 0, 1, ('dw', 'bwd_dw', 3, 1, 0, 1, 0, 0, 1, 0), ()),
    ('dw', 'bwd_dw', 1, 5, 5, 4, 3, 1, 0, 1, ('dw', 'bwd_dw', 3, 1, 0, 1, 0, 0, 1, 0), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0')),
    ('dw', 'bwd_dw', 1, 5, 1, 68, 3, 1, 0, 1, ('dw', 'bwd_dw', 3, 1, 0, 1, 0, 0, 1, 1), ()),
    ('dw', 'bwd_dw', 1, 5, 5, 68, 3, 1, 0, 1, ('dw', 'bwd_dw', 3, 1, 0, 1, 0, 0, 1, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'C > 64, C % 64 != 0')),
    ('dw', 'bwd_dw', 1, 1, 129, 4, 3, 1, 0, 1, ('dw', 'bwd_dw', 3, 1, 0, 1, 1, 0, 1, 0), ()),
    ('dw', 'bwd_dw', 1, 4, 49, 4, 3, 1, 0, 1, ('dw', 'bwd_dw', 3, 1, 0, 1, 1, 0, 1, 0), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'Wo > 48, Wo % 32 != 0')),
    ('dw', 'bwd_dw', 1, 1, 129, 68, 3, 1, 0, 1, ('dw', 'bwd_dw', 3, 1, 0, 1, 1, 0, 1, 1), ()),
    ('dw', 'bwd_dw', 1, 4, 49, 68, 3, 1, 0, 1, ('dw', 'bwd_dw', 3, 1, 0, 1, 1, 0, 1, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'C > 64, C % 64 != 0', 'Wo > 48, Wo % 32 != 0')),
    ('dw', 'bwd_dw', 2, 683, 65, 4, 3, 1, 0, 1, ('dw', 'bwd_dw', 3, 1, 0, 1, 1, 1, 1, 0), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'Wo > 48, Wo % 32 != 0')),
    ('dw', 'bwd_dw', 1, 683, 65, 68, 3, 1, 0, 1, ('dw', 'bwd_dw', 3, 1, 0, 1, 1, 1, 1, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'C > 64, C % 64 != 0', 'Wo > 48, Wo % 32 != 0')),
    ('dw', 'bwd_dw', 3, 3, 1, 68, 3, 2, 0, 0, ('dw', 'bwd_dw', 3, 2, 0, 0, 0, 0, 1, 1), ()),
    ('dw', 'bwd_dw', 1, 9, 5, 68, 3, 2, 0, 0, ('dw', 'bwd_dw', 3, 2, 0, 0, 0, 0, 1, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'odd H and W at stride 2', 'C > 64, C % 64 != 0')),
    ('dw', 'bwd_dw', 2, 1, 129, 68, 3, 2, 0, 0, ('dw', 'bwd_dw', 3, 2, 0, 0, 1, 0, 1, 1), ()),
    ('dw', 'bwd_dw', 1, 5, 97, 68, 3, 2, 0, 0, ('dw', 'bwd_dw', 3, 2, 0, 0, 1, 0, 1, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'odd H and W at stride 2', 'C > 64, C % 64 != 0', 'Wo > 48, Wo % 32 != 0')),
    ('dw', 'bwd_dw', 2, 683, 129, 68, 3, 2, 0, 0, ('dw', 'bwd_dw', 3, 2, 0, 0, 1, 1, 1, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'odd H and W at stride 2', 'C > 64, C % 64 != 0', 'Wo > 48, Wo % 32 != 0')),
    ('dw', 'bwd_dw', 3, 3, 1, 68, 3, 2, 1, 0, ('dw', 'bwd_dw', 3, 2, 1, 0, 0, 0, 1, 1), ()),
    ('dw', 'bwd_dw', 1, 9, 5, 68, 3, 2, 1, 0, ('dw', 'bwd_dw', 3, 2, 1, 0, 0, 0, 1, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'odd H and W at stride 2', 'C > 64, C % 64 != 0')),
    ('dw', 'bwd_dw', 2, 1, 129, 68, 3, 2, 1, 0, ('dw', 'bwd_dw', 3, 2, 1, 0, 1, 0, 1, 1), ()),
    ('dw', 'bwd_dw', 1, 5, 97, 68, 3, 2, 1, 0, ('dw', 'bwd_dw', 3, 2, 1, 0, 1, 0, 1, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'odd H and W at stride 2', 'C > 64, C % 64 != 0', 'Wo > 48, Wo % 32 != 0')),
    ('dw', 'bwd_dw', 2, 683, 129, 68, 3, 2, 1, 0, ('dw', 'bwd_dw', 3, 2, 1, 0, 1, 1, 1, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'odd H and W at stride 2', 'C > 64, C % 64 != 0', 'Wo > 48, Wo % 32 != 0')),
    ('dw', 'bwd_dw', 1, 5, 1, 68, 5, 1, 0, 0, ('dw', 'bwd_dw', 5, 1, 0, 0, 0, 0, 1, 1), ()),
    ('dw', 'bwd_dw', 1, 6, 6, 68, 5, 1, 0, 0, ('dw', 'bwd_dw', 5, 1, 0, 0, 0, 0, 1, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'C > 64, C % 64 != 0')),
    ('dw', 'bwd_dw', 3, 683, 1, 68, 5, 1, 0, 0, ('dw', 'bwd_dw', 5, 1, 0, 0, 0, 1, 1, 1), ()),
    ('dw', 'bwd_dw', 3, 683, 6, 68, 5, 1, 0, 0, ('dw', 'bwd_dw', 5, 1, 0, 0, 0, 1, 1, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'C > 64, C % 64 != 0')),
    ('dw', 'bwd_dw', 1, 1, 129, 68, 5, 1, 0, 0, ('dw', 'bwd_dw', 5, 1, 0, 0, 1, 0, 1, 1), ()),
    ('dw', 'bwd_dw', 1, 6, 49, 68, 5, 1, 0, 0, ('dw', 'bwd_dw', 5, 1, 0, 0, 1, 0, 1, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'C > 64, C % 64 != 0', 'Wo > 48, Wo % 32 != 0')),
    ('dw', 'bwd_dw', 1, 683, 65, 68, 5, 1, 0, 0, ('dw', 'bwd_dw', 5, 1, 0, 0, 1, 1, 1, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'C > 64, C % 64 != 0', 'Wo > 48, Wo % 32 != 0')),
    ('dw', 'bwd_dw', 3, 3, 1, 68, 5, 2, 0, 0, ('dw', 'bwd_dw', 5, 2, 0, 0, 0, 0, 1, 1), ()),
    ('dw', 'bwd_dw', 1, 9, 9, 68, 5, 2, 0, 0, ('dw', 'bwd_dw', 5, 2, 0, 0, 0, 0, 1, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'odd H and W at stride 2', 'C > 64, C % 64 != 0')),
    ('dw', 'bwd_dw', 1, 4097, 1, 68, 5, 2, 0, 0, ('dw', 'bwd_dw', 5, 2, 0, 0, 0, 1, 1, 1), ()),
    ('dw', 'bwd_dw', 1, 4097, 9, 68, 5, 2, 0, 0, ('dw', 'bwd_dw', 5, 2, 0, 0, 0, 1, 1, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'odd H and W at stride 2', 'C > 64, C % 64 != 0')),
    ('dw', 'bwd_dw', 2, 1, 129, 68, 5, 2, 0, 0, ('dw', 'bwd_dw', 5, 2, 0, 0, 1, 0, 1, 1), ()),
    ('dw', 'bwd_dw', 1, 7, 97, 68, 5, 2, 0, 0, ('dw', 'bwd_dw', 5, 2, 0, 0, 1, 0, 1, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'odd H and W at stride 2', 'C > 64, C % 64 != 0', 'Wo > 48, Wo % 32 != 0')),
    ('dw', 'bwd_dw', 2, 683, 129, 68, 5, 2, 0, 0, ('dw', 'bwd_dw', 5, 2, 0, 0, 1, 1, 1, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'odd H and W at stride 2', 'C > 64, C % 64 != 0', 'Wo > 48, Wo % 32 != 0')),
    ('dw', 'bwd_dw', 3, 3, 1, 68, 5, 2, 1, 0, ('dw', 'bwd_dw', 5, 2, 1, 0, 0, 0, 1, 1), ()),
    ('dw', 'bwd_dw', 1, 9, 9, 68, 5, 2, 1, 0, ('dw', 'bwd_dw', 5, 2, 1, 0, 0, 0, 1, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'odd H and W at stride 2', 'C > 64, C % 64 != 0')),
    ('dw', 'bwd_dw', 1, 4097, 1, 68, 5, 2, 1, 0, ('dw', 'bwd_dw', 5, 2, 1, 0, 0, 1, 1, 1), ()),
    ('dw', 'bwd_dw', 1, 4097, 9, 68, 5, 2, 1, 0, ('dw', 'bwd_dw', 5, 2, 1, 0, 0, 1, 1, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'odd H and W at stride 2', 'C > 64, C % 64 != 0')),
    ('dw', 'bwd_dw', 2, 1, 129, 68, 5, 2, 1, 0, ('dw', 'bwd_dw', 5, 2, 1, 0, 1, 0, 1, 1), ()),
    ('dw', 'bwd_dw', 1, 7, 97, 68, 5, 2, 1, 0, ('dw', 'bwd_dw', 5, 2, 1, 0, 1, 0, 1, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'odd H and W at stride 2', 'C > 64, C % 64 != 0', 'Wo > 48, Wo % 32 != 0')),
    ('dw', 'bwd_dw', 2, 683, 129, 68, 5, 2, 1, 0, ('dw', 'bwd_dw', 5, 2, 1, 0, 1, 1, 1, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'odd H and W at stride 2', 'C > 64, C % 64 != 0', 'Wo > 48, Wo % 32 != 0')),
    ('dw', 'bwd_dx', 2, 3, 43, 4, 3, 2, 0, 1, ('dw', 'bwd_dx', 0, 3, 2, 0, 1, 1), ()),
    ('dw', 'bwd_dx', 1, 5, 5, 68, 3, 2, 0, 1, ('dw', 'bwd_dx', 0, 3, 2, 0, 1, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'odd H and W at stride 2', 'C > 64, C % 64 != 0')),
    ('dw', 'bwd_dx', 2, 3, 43, 4, 3, 2, 1, 1, ('dw', 'bwd_dx', 0, 3, 2, 1, 1, 1), ()),
    ('dw', 'bwd_dx', 1, 5, 5, 68, 3, 2, 1, 1, ('dw', 'bwd_dx', 0, 3, 2, 1, 1, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'odd H and W at stride 2', 'C > 64, C % 64 != 0')),
    ('dw', 'bwd_dx', 2, 3, 43, 4, 5, 2, 0, 1, ('dw', 'bwd_dx', 0, 5, 2, 0, 1, 1), ()),
    ('dw', 'bwd_dx', 1, 7, 9, 68, 5, 2, 0, 1, ('dw', 'bwd_dx', 0, 5, 2, 0, 1, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'odd H and W at stride 2', 'C > 64, C % 64 != 0')),
    ('dw', 'bwd_dx', 2, 3, 43, 4, 5, 2, 1, 1, ('dw', 'bwd_dx', 0, 5, 2, 1, 1, 1), ()),
    ('dw', 'bwd_dx', 1, 7, 9, 68, 5, 2, 1, 1, ('dw', 'bwd_dx', 0, 5, 2, 1, 1, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'odd H and W at stride 2', 'C > 64, C % 64 != 0')),
    ('dw', 'bwd_dx', 1, 1, 1, 4, 3, 1, 0, 0, ('dw', 'bwd_dx', 1, 3, 1, 0, 0, 0), ()),
    ('dw', 'bwd_dx', 1, 4, 5, 68, 3, 1, 0, 0, ('dw', 'bwd_dx', 1, 3, 1, 0, 0, 0), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'C > 64, C % 64 != 0')),
    ('dw', 'bwd_dx', 3, 43, 1, 8, 3, 1, 0, 0, ('dw', 'bwd_dx', 1, 3, 1, 0, 0, 1), ()),
    ('dw', 'bwd_dx', 1, 4, 5, 132, 3, 1, 0, 0, ('dw', 'bwd_dx', 1, 3, 1, 0, 0, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'C > 64, C % 64 != 0')),
    ('dw', 'bwd_dx', 3, 43, 1, 8, 3, 1, 0, 1, ('dw', 'bwd_dx', 1, 3, 1, 0, 1, 1), ()),
    ('dw', 'bwd_dx', 1, 4, 5, 132, 3, 1, 0, 1, ('dw', 'bwd_dx', 1, 3, 1, 0, 1, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'C > 64, C % 64 != 0')),
    ('dw', 'bwd_dx', 3, 43, 1, 8, 5, 1, 0, 1, ('dw', 'bwd_dx', 1, 5, 1, 0, 1, 1), ()),
    ('dw', 'bwd_dx', 1, 8, 6, 68, 5, 1, 0, 1, ('dw', 'bwd_dx', 1, 5, 1, 0, 1, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'C > 64, C % 64 != 0')),
    ('dw', 'fwd', 1, 4, 4, 4, 3, 1, 0, 0, ('dw', 'fwd', 3, 1, 0, 0, 0, 0, 0), ('H > k and W > k',)),
    ('dw', 'fwd', 1, 1, 1, 4, 3, 1, 0, 0, ('dw', 'fwd', 3, 1, 0, 0, 0, 0, 0), ('W % 4 != 0 and Wo % 4 != 0',)),
    ('dw', 'fwd', 1, 4, 4, 68, 3, 1, 0, 0, ('dw', 'fwd', 3, 1, 0, 0, 0, 0, 1), ('H > k and W > k',)),
    ('dw', 'fwd', 1, 1, 1, 68, 3, 1, 0, 0, ('dw', 'fwd', 3, 1, 0, 0, 0, 0, 1), ('W % 4 != 0 and Wo % 4 != 0', 'C > 64, C % 64 != 0')),
    ('dw', 'fwd', 1, 1, 5, 4, 3, 1, 0, 0, ('dw', 'fwd', 3, 1, 0, 0, 0, 1, 0), ()),
    ('dw', 'fwd', 1, 4, 5, 4, 3, 1, 0, 0, ('dw', 'fwd', 3, 1, 0, 0, 0, 1, 0), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0')),
    ('dw', 'fwd', 1, 1, 5, 68, 3, 1, 0, 0, ('dw', 'fwd', 3, 1, 0, 0, 0, 1, 1), ()),
    ('dw', 'fwd', 1, 4, 5, 68, 3, 1, 0, 0, ('dw', 'fwd', 3, 1, 0, 0, 0, 1, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'C > 64, C % 64 != 0')),
    ('dw', 'fwd', 1, 65, 5, 4, 3, 1, 0, 0, ('dw', 'fwd', 3, 1, 0, 0, 1, 1, 0), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'ragged last block of an image')),
    ('dw', 'fwd', 1, 65, 5, 68, 3, 1, 0, 0, ('dw', 'fwd', 3, 1, 0, 0, 1, 1, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'C > 64, C % 64 != 0', 'ragged last block of an image')),
    ('dw', 'fwd', 1, 4, 4, 68, 3, 1, 0, 1, ('dw', 'fwd', 3, 1, 0, 1, 0, 0, 1), ('H > k and W > k',)),
    ('dw', 'fwd', 1, 1, 1, 68, 3, 1, 0, 1, ('dw', 'fwd', 3, 1, 0, 1, 0, 0, 1), ('W % 4 != 0 and Wo % 4 != 0', 'C > 64, C % 64 != 0')),
    ('dw', 'fwd', 1, 1, 5, 68, 3, 1, 0, 1, ('dw', 'fwd', 3, 1, 0, 1, 0, 1, 1), ()),
    ('dw', 'fwd', 1, 4, 5, 68, 3, 1, 0, 1, ('dw', 'fwd', 3, 1, 0, 1, 0, 1, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'C > 64, C % 64 != 0')),
    ('dw', 'fwd', 1, 65, 5, 4, 3, 1, 0, 1, ('dw', 'fwd', 3, 1, 0, 1, 1, 1, 0), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'ragged last block of an image')),
    ('dw', 'fwd', 1, 65, 5, 68, 3, 1, 0, 1, ('dw', 'fwd', 3, 1, 0, 1, 1, 1, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'C > 64, C % 64 != 0', 'ragged last block of an image')),
    ('dw', 'fwd', 1, 1, 9, 68, 3, 2, 0, 1, ('dw', 'fwd', 3, 2, 0, 1, 0, 1, 1), ()),
    ('dw', 'fwd', 1, 5, 9, 68, 3, 2, 0, 1, ('dw', 'fwd', 3, 2, 0, 1, 0, 1, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'odd H and W at stride 2', 'C > 64, C % 64 != 0')),
    ('dw', 'fwd', 1, 65, 25, 68, 3, 2, 0, 1, ('dw', 'fwd', 3, 2, 0, 1, 1, 1, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'odd H and W at stride 2', 'C > 64, C % 64 != 0', 'ragged last block of an image')),
    ('dw', 'fwd', 1, 1, 9, 68, 3, 2, 1, 1, ('dw', 'fwd', 3, 2, 1, 1, 0, 1, 1), ()),
    ('dw', 'fwd', 1, 5, 9, 68, 3, 2, 1, 1, ('dw', 'fwd', 3, 2, 1, 1, 0, 1, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'odd H and W at stride 2', 'C > 64, C % 64 != 0')),
    ('dw', 'fwd', 1, 65, 25, 68, 3, 2, 1, 1, ('dw', 'fwd', 3, 2, 1, 1, 1, 1, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'odd H and W at stride 2', 'C > 64, C % 64 != 0', 'ragged last block of an image')),
    ('dw', 'fwd', 1, 1, 1, 68, 5, 1, 0, 1, ('dw', 'fwd', 5, 1, 0, 1, 0, 0, 1), ('W % 4 != 0 and Wo % 4 != 0', 'C > 64, C % 64 != 0')),
    ('dw', 'fwd', 1, 1, 5, 68, 5, 1, 0, 1, ('dw', 'fwd', 5, 1, 0, 1, 0, 1, 1), ()),
    ('dw', 'fwd', 1, 6, 6, 68, 5, 1, 0, 1, ('dw', 'fwd', 5, 1, 0, 1, 0, 1, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'C > 64, C % 64 != 0')),
    ('dw', 'fwd', 1, 65, 5, 68, 5, 1, 0, 1, ('dw', 'fwd', 5, 1, 0, 1, 1, 1, 1), ()),
    ('dw', 'fwd', 1, 43, 9, 68, 5, 1, 0, 1, ('dw', 'fwd', 5, 1, 0, 1, 1, 1, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'C > 64, C % 64 != 0', 'ragged last block of an image')),
    ('dw', 'fwd', 1, 6, 6, 68, 5, 2, 0, 1, ('dw', 'fwd', 5, 2, 0, 1, 0, 0, 1), ('H > k and W > k',)),
    ('dw', 'fwd', 1, 1, 1, 68, 5, 2, 0, 1, ('dw', 'fwd', 5, 2, 0, 1, 0, 0, 1), ('W % 4 != 0 and Wo % 4 != 0', 'odd H and W at stride 2', 'C > 64, C % 64 != 0')),
    ('dw', 'fwd', 1, 1, 9, 68, 5, 2, 0, 1, ('dw', 'fwd', 5, 2, 0, 1, 0, 1, 1), ()),
    ('dw', 'fwd', 1, 7, 9, 68, 5, 2, 0, 1, ('dw', 'fwd', 5, 2, 0, 1, 0, 1, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'odd H and W at stride 2', 'C > 64, C % 64 != 0')),
    ('dw', 'fwd', 1, 65, 25, 68, 5, 2, 0, 1, ('dw', 'fwd', 5, 2, 0, 1, 1, 1, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'odd H and W at stride 2', 'C > 64, C % 64 != 0', 'ragged last block of an image')),
    ('dw', 'fwd', 1, 6, 6, 68, 5, 2, 1, 1, ('dw', 'fwd', 5, 2, 1, 1, 0, 0, 1), ('H > k and W > k',)),
    ('dw', 'fwd', 1, 1, 1, 68, 5, 2, 1, 1, ('dw', 'fwd', 5, 2, 1, 1, 0, 0, 1), ('W % 4 != 0 and Wo % 4 != 0', 'odd H and W at stride 2', 'C > 64, C % 64 != 0')),
    ('dw', 'fwd', 1, 1, 9, 68, 5, 2, 1, 1, ('dw', 'fwd', 5, 2, 1, 1, 0, 1, 1), ()),
    ('dw', 'fwd', 1, 7, 9, 68, 5, 2, 1, 1, ('dw', 'fwd', 5, 2, 1, 1, 0, 1, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'odd H and W at stride 2', 'C > 64, C % 64 != 0')),
    ('dw', 'fwd', 1, 65, 25, 68, 5, 2, 1, 1, ('dw', 'fwd', 5, 2, 1, 1, 1, 1, 1), ('H > k and W > k', 'W % 4 != 0 and Wo % 4 != 0', 'odd H and W at stride 2', 'C > 64, C % 64 != 0', 'ragged last block of an image')),
    ('nt', 'gemm_nt_levels', 1, 1, 4, 2, 0, (0, 1, 1), (1, ((1, 1),)), 0, 0, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 1, 1, 0, 0, 4, 0, 2, 0), ()),
    ('nt', 'gemm_nt_levels', 162, 49, 68, 2, 0, (0, 3969, 49), (2, ((10, 6), (5, 3), (3, 2))), 0, 0, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 1, 1, 0, 0, 4, 0, 2, 0), ('M % 128 and M % 32 != 0, last wave without a row', 'N > 64, N % 64 != 0', 'N % 16 a non-zero multiple of 4', 'K % 16 != 0', 'K > 32, K % 32 > 16')),
    ('nt', 'gemm_nt_levels', 1, 2, 4, 2, 0, (0, 2, 2), (1, ((1, 1),)), 0, 0, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 2, 1, 0, 0, 4, 0, 2, 0), ()),
    ('nt', 'gemm_nt_levels', 162, 50, 68, 2, 0, (0, 4050, 50), (2, ((10, 6), (5, 3), (3, 2))), 0, 0, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 2, 1, 0, 0, 4, 0, 2, 0), ('M % 128 and M % 32 != 0, last wave without a row', 'N > 64, N % 64 != 0', 'N % 16 a non-zero multiple of 4', 'K % 16 != 0', 'K > 32, K % 32 > 16')),
    ('nt', 'gemm_nt_relu', 1, 2, 4, 0, 0, (0, 0, 0), None, 0, 0, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 2, 1, 0, 1, 4, 0, 0, 0), ()),
    ('nt', 'gemm_nt_relu', 129, 50, 68, 0, 0, (0, 0, 0), None, 0, 0, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 2, 1, 0, 1, 4, 0, 0, 0), ('M % 128 and M % 32 != 0, last wave without a row', 'N > 64, N % 64 != 0', 'N % 16 a non-zero multiple of 4', 'K % 16 != 0', 'K > 32, K % 32 > 16')),
    ('nt', 'gemm_nt_levels', 162, 386, 68, 2, 0, (0, 31266, 386), (2, ((10, 6), (5, 3), (3, 2))), 0, 0, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 2, 4, 0, 0, 4, 0, 2, 0), ('M % 128 and M % 32 != 0, last wave without a row', 'N > 64, N % 64 != 0', 'N % 16 a non-zero multiple of 4', 'K % 16 != 0', 'split-K, K % 64 != 0')),
    ('nt', 'gemm_nt_levels', 1, 384, 4, 2, 0, (0, 386, 386), (1, ((1, 1),)), 0, 0, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 2, 4, 0, 0, 4, 0, 2, 0), ('split-K, K % 64 == 0',)),
    ('nt', 'gemm_nt_levels', 1, 4, 4, 2, 0, (0, 4, 4), (1, ((1, 1),)), 0, 0, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 4, 1, 0, 0, 4, 0, 2, 0), ()),
    ('nt', 'gemm_nt_levels', 162, 52, 68, 2, 0, (0, 4212, 52), (2, ((10, 6), (5, 3), (3, 2))), 0, 0, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 4, 1, 0, 0, 4, 0, 2, 0), ('M % 128 and M % 32 != 0, last wave without a row', 'N > 64, N % 64 != 0', 'N % 16 a non-zero multiple of 4', 'K % 16 != 0', 'K > 32, K % 32 > 16')),
    ('nt', 'gemm_nt_levels', 162, 52, 65, 0, 2, (0, 5427, 67), (2, ((10, 6), (5, 3), (3, 2))), 1, 0, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 4, 1, 1, 0, 0, 1, 0, 2), ('M % 128 and M % 32 != 0, last wave without a row', 'N > 64, N % 64 != 0', 'N odd', 'K % 16 != 0', 'K > 32, K % 32 > 16', 'C rows with ld > N')),
    ('nt', 'gemm_nt_levels', 1, 4, 1, 0, 2, (0, 1, 1), (1, ((1, 1),)), 1, 0, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 4, 1, 1, 0, 0, 1, 0, 2), ('K == 4',)),
    ('nt', 'gemm_nt_levels', 162, 52, 66, 0, 2, (0, 5508, 68), (2, ((10, 6), (5, 3), (3, 2))), 1, 0, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 4, 1, 1, 0, 2, 1, 0, 2), ('M % 128 and M % 32 != 0, last wave without a row', 'N > 64, N % 64 != 0', 'N % 16 == 2', 'K % 16 != 0', 'K > 32, K % 32 > 16', 'C rows with ld > N')),
    ('nt', 'gemm_nt_levels', 1, 4, 2, 0, 2, (0, 2, 2), (1, ((1, 1),)), 1, 0, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 4, 1, 1, 0, 2, 1, 0, 2), ('K == 4',)),
    ('nt', 'gemm_nt', 129, 52, 68, 0, 0, (0, 0, 0), None, 0, 0, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 4, 1, 1, 0, 4, 0, 0, 0), ('M % 128 and M % 32 != 0, last wave without a row', 'N > 64, N % 64 != 0', 'N % 16 a non-zero multiple of 4', 'K % 16 != 0', 'K > 32, K % 32 > 16')),
    ('nt', 'gemm_nt', 1, 4, 4, 0, 0, (0, 0, 0), None, 0, 0, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 4, 1, 1, 0, 4, 0, 0, 0), ('K == 4',)),
    ('nt', 'gemm_nt', 129, 52, 68, 0, 0, (0, 0, 0), None, 1, 0, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 4, 1, 1, 0, 4, 1, 0, 0), ('M % 128 and M % 32 != 0, last wave without a row', 'N > 64, N % 64 != 0', 'N % 16 a non-zero multiple of 4', 'K % 16 != 0', 'K > 32, K % 32 > 16')),
    ('nt', 'gemm_nt', 1, 4, 4, 0, 0, (0, 0, 0), None, 1, 0, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 4, 1, 1, 0, 4, 1, 0, 0), ('K == 4',)),
    ('nt', 'gemm_nt_levels', 162, 52, 68, 0, 2, (0, 5832, 72), (2, ((10, 6), (5, 3), (3, 2))), 1, 0, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 4, 1, 1, 0, 4, 1, 0, 2), ('M % 128 and M % 32 != 0, last wave without a row', 'N > 64, N % 64 != 0', 'N % 16 a non-zero multiple of 4', 'K % 16 != 0', 'K > 32, K % 32 > 16', 'C rows with ld > N')),
    ('nt', 'gemm_nt_levels', 1, 4, 4, 0, 2, (0, 4, 4), (1, ((1, 1),)), 1, 0, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 4, 1, 1, 0, 4, 1, 0, 2), ('K == 4',)),
    ('nt', 'gemm_nt_fused', 129, 52, 68, 0, 0, (0, 0, 0), None, 11, 20, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 4, 1, 1, 0, 4, 11, 0, 0), ('M % 128 and M % 32 != 0, last wave without a row', 'N > 64, N % 64 != 0', 'N % 16 a non-zero multiple of 4', 'K % 16 != 0', 'K > 32, K % 32 > 16', 'gate rows not dividing 32')),
    ('nt', 'gemm_nt_fused', 1, 4, 4, 0, 0, (0, 0, 0), None, 11, 1, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 4, 1, 1, 0, 4, 11, 0, 0), ('K == 4',)),
    ('nt', 'gemm_nt_fused', 129, 52, 68, 0, 0, (0, 0, 0), None, 2, 0, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 4, 1, 1, 0, 4, 2, 0, 0), ('M % 128 and M % 32 != 0, last wave without a row', 'N > 64, N % 64 != 0', 'N % 16 a non-zero multiple of 4', 'K % 16 != 0', 'K > 32, K % 32 > 16')),
    ('nt', 'gemm_nt_fused', 1, 4, 4, 0, 0, (0, 0, 0), None, 2, 0, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 4, 1, 1, 0, 4, 2, 0, 0), ('K == 4',)),
    ('nt', 'gemm_nt_fused', 129, 52, 68, 0, 0, (0, 0, 0), None, 5, 0, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 4, 1, 1, 0, 4, 5, 0, 0), ('M % 128 and M % 32 != 0, last wave without a row', 'N > 64, N % 64 != 0', 'N % 16 a non-zero multiple of 4', 'K % 16 != 0', 'K > 32, K % 32 > 16')),
    ('nt', 'gemm_nt_fused', 1, 4, 4, 0, 0, (0, 0, 0), None, 5, 0, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 4, 1, 1, 0, 4, 5, 0, 0), ('K == 4',)),
    ('nt', 'gemm_nt_fused', 129, 52, 68, 0, 0, (0, 0, 0), None, 9, 20, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 4, 1, 1, 0, 4, 9, 0, 0), ('M % 128 and M % 32 != 0, last wave without a row', 'N > 64, N % 64 != 0', 'N % 16 a non-zero multiple of 4', 'K % 16 != 0', 'K > 32, K % 32 > 16', 'gate rows not dividing 32')),
    ('nt', 'gemm_nt_fused', 1, 4, 4, 0, 0, (0, 0, 0), None, 9, 1, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 4, 1, 1, 0, 4, 9, 0, 0), ('K == 4',)),
    ('nt', 'gemm_nt_relu', 129, 52, 68, 0, 0, (0, 0, 0), None, 0, 0, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 4, 1, 1, 1, 4, 0, 0, 0), ('M % 128 and M % 32 != 0, last wave without a row', 'N > 64, N % 64 != 0', 'N % 16 a non-zero multiple of 4', 'K % 16 != 0', 'K > 32, K % 32 > 16')),
    ('nt', 'gemm_nt_relu', 1, 4, 4, 0, 0, (0, 0, 0), None, 0, 0, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 4, 1, 1, 1, 4, 0, 0, 0), ('K == 4',)),
    ('nt', 'gemm_nt_mask', 129, 52, 68, 0, 0, (0, 0, 0), None, 32, 0, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 4, 1, 1, 2, 4, 32, 0, 0), ('M % 128 and M % 32 != 0, last wave without a row', 'N > 64, N % 64 != 0', 'N % 16 a non-zero multiple of 4', 'K % 16 != 0', 'K > 32, K % 32 > 16')),
    ('nt', 'gemm_nt_mask', 1, 4, 4, 0, 0, (0, 0, 0), None, 32, 0, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 4, 1, 1, 2, 4, 32, 0, 0), ('K == 4',)),
    ('nt', 'gemm_nt_fused', 129, 388, 68, 0, 0, (0, 0, 0), None, 0, 0, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 4, 4, 1, 0, 4, 0, 0, 0), ('M % 128 and M % 32 != 0, last wave without a row', 'N > 64, N % 64 != 0', 'N % 16 a non-zero multiple of 4', 'K % 16 != 0', 'split-K, K % 64 != 0')),
    ('nt', 'gemm_nt_fused', 1, 384, 4, 0, 0, (0, 0, 0), None, 0, 0, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 4, 4, 1, 0, 4, 0, 0, 0), ('split-K, K % 64 == 0',)),
    ('nt', 'gemm_nt', 129, 388, 68, 0, 0, (0, 0, 0), None, 1, 0, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 4, 4, 1, 0, 4, 1, 0, 0), ('M % 128 and M % 32 != 0, last wave without a row', 'N > 64, N % 64 != 0', 'N % 16 a non-zero multiple of 4', 'K % 16 != 0', 'split-K, K % 64 != 0')),
    ('nt', 'gemm_nt', 1, 384, 4, 0, 0, (0, 0, 0), None, 1, 0, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 4, 4, 1, 0, 4, 1, 0, 0), ('split-K, K % 64 == 0',)),
    ('nt', 'gemm_nt_fused', 129, 388, 68, 0, 0, (0, 0, 0), None, 11, 20, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 4, 4, 1, 0, 4, 11, 0, 0), ('M % 128 and M % 32 != 0, last wave without a row', 'N > 64, N % 64 != 0', 'N % 16 a non-zero multiple of 4', 'K % 16 != 0', 'split-K, K % 64 != 0', 'gate rows not dividing 32')),
    ('nt', 'gemm_nt_fused', 1, 384, 4, 0, 0, (0, 0, 0), None, 11, 1, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 4, 4, 1, 0, 4, 11, 0, 0), ('split-K, K % 64 == 0',)),
    ('nt', 'gemm_nt_fused', 129, 388, 68, 0, 0, (0, 0, 0), None, 2, 0, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 4, 4, 1, 0, 4, 2, 0, 0), ('M % 128 and M % 32 != 0, last wave without a row', 'N > 64, N % 64 != 0', 'N % 16 a non-zero multiple of 4', 'K % 16 != 0', 'split-K, K % 64 != 0')),
    ('nt', 'gemm_nt_fused', 1, 384, 4, 0, 0, (0, 0, 0), None, 2, 0, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 4, 4, 1, 0, 4, 2, 0, 0), ('split-K, K % 64 == 0',)),
    ('nt', 'gemm_nt_fused', 129, 388, 68, 0, 0, (0, 0, 0), None, 5, 0, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 4, 4, 1, 0, 4, 5, 0, 0), ('M % 128 and M % 32 != 0, last wave without a row', 'N > 64, N % 64 != 0', 'N % 16 a non-zero multiple of 4', 'K % 16 != 0', 'split-K, K % 64 != 0')),
    ('nt', 'gemm_nt_fused', 1, 384, 4, 0, 0, (0, 0, 0), None, 5, 0, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 4, 4, 1, 0, 4, 5, 0, 0), ('split-K, K % 64 == 0',)),
    ('nt', 'gemm_nt_fused', 129, 388, 68, 0, 0, (0, 0, 0), None, 9, 20, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 4, 4, 1, 0, 4, 9, 0, 0), ('M % 128 and M % 32 != 0, last wave without a row', 'N > 64, N % 64 != 0', 'N % 16 a non-zero multiple of 4', 'K % 16 != 0', 'split-K, K % 64 != 0', 'gate rows not dividing 32')),
    ('nt', 'gemm_nt_fused', 1, 384, 4, 0, 0, (0, 0, 0), None, 9, 1, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 4, 4, 1, 0, 4, 9, 0, 0), ('split-K, K % 64 == 0',)),
    ('nt', 'gemm_nt_relu', 129, 388, 68, 0, 0, (0, 0, 0), None, 0, 0, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 4, 4, 1, 1, 4, 0, 0, 0), ('M % 128 and M % 32 != 0, last wave without a row', 'N > 64, N % 64 != 0', 'N % 16 a non-zero multiple of 4', 'K % 16 != 0', 'split-K, K % 64 != 0')),
    ('nt', 'gemm_nt_relu', 1, 384, 4, 0, 0, (0, 0, 0), None, 0, 0, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 4, 4, 1, 1, 4, 0, 0, 0), ('split-K, K % 64 == 0',)),
    ('nt', 'gemm_nt_mask', 129, 388, 68, 0, 0, (0, 0, 0), None, 32, 0, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 4, 4, 1, 2, 4, 32, 0, 0), ('M % 128 and M % 32 != 0, last wave without a row', 'N > 64, N % 64 != 0', 'N % 16 a non-zero multiple of 4', 'K % 16 != 0', 'split-K, K % 64 != 0')),
    ('nt', 'gemm_nt_mask', 1, 384, 4, 0, 0, (0, 0, 0), None, 32, 0, (0, 0, 0, 0, 0, 0, 0, 0), ('nt', 4, 4, 1, 2, 4, 32, 0, 0), ('split-K, K % 64 == 0',)),
    ('tn', 'gemm_tn_levels', 341, 1, 64, 2, (0, 341, 1), (1, ((16, 16), (8, 8), (4, 4), (2, 2), (1, 1))), 0, (0, 0, 0), ('tn', 0, 1, 1, 0, 0, 2, 1), ('M % 32 != 0, M no multiple of rows_per_slice', 'N % 32 != 0', 'K % 64 == 0')),
    ('tn', 'gemm_tn_levels', 341, 1, 60, 2, (0, 341, 1), (1, ((16, 16), (8, 8), (4, 4), (2, 2), (1, 1))), 0, (0, 0, 0), ('tn', 0, 1, 1, 0, 0, 2, 1), ('M % 32 != 0, M no multiple of rows_per_slice', 'N % 32 != 0', 'K % 64 == 60')),
    ('tn', 'gemm_tn_levels', 341, 1, 4, 2, (0, 341, 1), (1, ((16, 16), (8, 8), (4, 4), (2, 2), (1, 1))), 0, (0, 0, 0), ('tn', 0, 1, 1, 0, 0, 2, 1), ('M % 32 != 0, M no multiple of rows_per_slice', 'N % 32 != 0', 'K % 64 neither 0 nor 60')),
    ('tn', 'gemm_tn_levels', 6742, 243, 256, 2, (0, 819153, 243), (2, ((58, 58), (3, 2), (1, 1))), 0, (0, 0, 0), ('tn', 0, 1, 1, 0, 0, 2, 2), ('M % 32 != 0, M no multiple of rows_per_slice', 'an empty trailing slice', 'N % 32 != 0', 'K % 64 == 0')),
    ('tn', 'gemm_tn_levels', 4130, 243, 508, 2, (0, 501795, 243), (2, ((41, 37), (21, 19), (11, 10), (6, 5), (3, 3))), 0, (0, 0, 0), ('tn', 0, 1, 1, 0, 0, 2, 2), ('M % 32 != 0, M no multiple of rows_per_slice', 'an empty trailing slice', 'N % 32 != 0', 'K % 64 == 60')),
    ('tn', 'gemm_tn_levels', 6742, 243, 260, 2, (0, 819153, 243), (2, ((58, 58), (3, 2), (1, 1))), 0, (0, 0, 0), ('tn', 0, 1, 1, 0, 0, 2, 2), ('M % 32 != 0, M no multiple of rows_per_slice', 'an empty trailing slice', 'N % 32 != 0', 'K % 64 neither 0 nor 60')),
    ('tn', 'gemm_tn_levels', 341, 2, 64, 2, (0, 682, 2), (1, ((16, 16), (8, 8), (4, 4), (2, 2), (1, 1))), 0, (0, 0, 0), ('tn', 1, 2, 1, 0, 0, 2, 1), ('M % 32 != 0, M no multiple of rows_per_slice', 'N % 32 != 0', 'K % 64 == 0')),
    ('tn', 'gemm_tn_levels', 341, 2, 60, 2, (0, 682, 2), (1, ((16, 16), (8, 8), (4, 4), (2, 2), (1, 1))), 0, (0, 0, 0), ('tn', 1, 2, 1, 0, 0, 2, 1), ('M % 32 != 0, M no multiple of rows_per_slice', 'N % 32 != 0', 'K % 64 == 60')),
    ('tn', 'gemm_tn_levels', 341, 2, 4, 2, (0, 682, 2), (1, ((16, 16), (8, 8), (4, 4), (2, 2), (1, 1))), 0, (0, 0, 0), ('tn', 1, 2, 1, 0, 0, 2, 1), ('M % 32 != 0, M no multiple of rows_per_slice', 'N % 32 != 0', 'K % 64 neither 0 nor 60')),
    ('tn', 'gemm_tn_levels', 6742, 250, 256, 2, (0, 842750, 250), (2, ((58, 58), (3, 2), (1, 1))), 0, (0, 0, 0), ('tn', 1, 2, 1, 0, 0, 2, 2), ('M % 32 != 0, M no multiple of rows_per_slice', 'an empty trailing slice', 'N % 32 != 0', 'K % 64 == 0')),
    ('tn', 'gemm_tn_levels', 4130, 250, 508, 2, (0, 516250, 250), (2, ((41, 37), (21, 19), (11, 10), (6, 5), (3, 3))), 0, (0, 0, 0), ('tn', 1, 2, 1, 0, 0, 2, 2), ('M % 32 != 0, M no multiple of rows_per_slice', 'an empty trailing slice', 'N % 32 != 0', 'K % 64 == 60')),
    ('tn', 'gemm_tn_levels', 6742, 250, 260, 2, (0, 842750, 250), (2, ((58, 58), (3, 2), (1, 1))), 0, (0, 0, 0), ('tn', 1, 2, 1, 0, 0, 2, 2), ('M % 32 != 0, M no multiple of rows_per_slice', 'an empty trailing slice', 'N % 32 != 0', 'K % 64 neither 0 nor 60')),
    ('tn', 'gemm_tn_levels', 341, 4, 64, 2, (0, 1364, 4), (1, ((16, 16), (8, 8), (4, 4), (2, 2), (1, 1))), 0, (0, 0, 0), ('tn', 1, 4, 1, 0, 0, 2, 1), ('M % 32 != 0, M no multiple of rows_per_slice', 'N % 32 != 0', 'K % 64 == 0')),
    ('tn', 'gemm_tn_levels', 341, 4, 60, 2, (0, 1364, 4), (1, ((16, 16), (8, 8), (4, 4), (2, 2), (1, 1))), 0, (0, 0, 0), ('tn', 1, 4, 1, 0, 0, 2, 1), ('M % 32 != 0, M no multiple of rows_per_slice', 'N % 32 != 0', 'K % 64 == 60')),
    ('tn', 'gemm_tn_levels', 341, 4, 4, 2, (0, 1364, 4), (1, ((16, 16), (8, 8), (4, 4), (2, 2), (1, 1))), 0, (0, 0, 0), ('tn', 1, 4, 1, 0, 0, 2, 1), ('M % 32 != 0, M no multiple of rows_per_slice', 'N % 32 != 0', 'K % 64 neither 0 nor 60')),
    ('tn', 'gemm_tn_levels', 6742, 252, 256, 2, (0, 849492, 252), (2, ((58, 58), (3, 2), (1, 1))), 0, (0, 0, 0), ('tn', 1, 4, 1, 0, 0, 2, 2), ('M % 32 != 0, M no multiple of rows_per_slice', 'an empty trailing slice', 'N % 32 != 0', 'K % 64 == 0')),
    ('tn', 'gemm_tn_levels', 4130, 252, 508, 2, (0, 520380, 252), (2, ((41, 37), (21, 19), (11, 10), (6, 5), (3, 3))), 0, (0, 0, 0), ('tn', 1, 4, 1, 0, 0, 2, 2), ('M % 32 != 0, M no multiple of rows_per_slice', 'an empty trailing slice', 'N % 32 != 0', 'K % 64 == 60')),
    ('tn', 'gemm_tn_levels', 6742, 252, 260, 2, (0, 849492, 252), (2, ((58, 58), (3, 2), (1, 1))), 0, (0, 0, 0), ('tn', 1, 4, 1, 0, 0, 2, 2), ('M % 32 != 0, M no multiple of rows_per_slice', 'an empty trailing slice', 'N % 32 != 0', 'K % 64 neither 0 nor 60')),
    ('tn', 'gemm_tn', 1, 4, 64, 0, (0, 0, 0), None, 0, (0, 0, 0), ('tn', 1, 4, 1, 1, 0, 0, 0), ('M % 32 != 0, M no multiple of rows_per_slice', 'N % 32 != 0', 'K % 64 == 0')),
    ('tn', 'gemm_tn', 1, 4, 60, 0, (0, 0, 0), None, 0, (0, 0, 0), ('tn', 1, 4, 1, 1, 0, 0, 0), ('M % 32 != 0, M no multiple of rows_per_slice', 'N % 32 != 0', 'K % 64 == 60')),
    ('tn', 'gemm_tn', 1, 4, 4, 0, (0, 0, 0), None, 0, (0, 0, 0), ('tn', 1, 4, 1, 1, 0, 0, 0), ('M % 32 != 0, M no multiple of rows_per_slice', 'N % 32 != 0', 'K % 64 neither 0 nor 60')),
    ('tn', 'gemm_tn', 257, 4, 64, 0, (0, 0, 0), None, 0, (0, 0, 0), ('tn', 1, 4, 1, 1, 0, 0, 1), ('M % 32 != 0, M no multiple of rows_per_slice', 'N % 32 != 0', 'K % 64 == 0')),
    ('tn', 'gemm_tn', 257, 4, 60, 0, (0, 0, 0), None, 0, (0, 0, 0), ('tn', 1, 4, 1, 1, 0, 0, 1), ('M % 32 != 0, M no multiple of rows_per_slice', 'N % 32 != 0', 'K % 64 == 60')),
    ('tn', 'gemm_tn', 257, 4, 4, 0, (0, 0, 0), None, 0, (0, 0, 0), ('tn', 1, 4, 1, 1, 0, 0, 1), ('M % 32 != 0, M no multiple of rows_per_slice', 'N % 32 != 0', 'K % 64 neither 0 nor 60')),
    ('tn', 'gemm_tn', 6657, 252, 256, 0, (0, 0, 0), None, 0, (0, 0, 0), ('tn', 1, 4, 1, 1, 0, 0, 2), ('M % 32 != 0, M no multiple of rows_per_slice', 'an empty trailing slice', 'N % 32 != 0', 'K % 64 == 0')),
    ('tn', 'gemm_tn', 8193, 252, 252, 0, (0, 0, 0), None, 0, (0, 0, 0), ('tn', 1, 4, 1, 1, 0, 0, 2), ('M % 32 != 0, M no multiple of rows_per_slice', 'an empty trailing slice', 'N % 32 != 0', 'K % 64 == 60')),
    ('tn', 'gemm_tn', 6657, 252, 260, 0, (0, 0, 0), None, 0, (0, 0, 0), ('tn', 1, 4, 1, 1, 0, 0, 2), ('M % 32 != 0, M no multiple of rows_per_slice', 'an empty trailing slice', 'N % 32 != 0', 'K % 64 neither 0 nor 60')),
    ('tn', 'gemm_tn_scaled', 1, 4, 4, 0, (0, 0, 0), None, 1, (0, 0, 0), ('tn', 1, 4, 1, 1, 1, 0, 0), ()),
    ('tn', 'gemm_tn_scaled', 10, 4, 64, 0, (0, 0, 0), None, 5, (0, 0, 0), ('tn', 1, 4, 1, 1, 1, 0, 0), ('M % 32 != 0, M no multiple of rows_per_slice', 'N % 32 != 0', 'K % 64 == 0', 'gate rows not dividing 16')),
    ('tn', 'gemm_tn_scaled', 10, 4, 60, 0, (0, 0, 0), None, 5, (0, 0, 0), ('tn', 1, 4, 1, 1, 1, 0, 0), ('M % 32 != 0, M no multiple of rows_per_slice', 'N % 32 != 0', 'K % 64 == 60', 'gate rows not dividing 16')),
    ('tn', 'gemm_tn_scaled', 10, 4, 4, 0, (0, 0, 0), None, 5, (0, 0, 0), ('tn', 1, 4, 1, 1, 1, 0, 0), ('M % 32 != 0, M no multiple of rows_per_slice', 'N % 32 != 0', 'K % 64 neither 0 nor 60', 'gate rows not dividing 16')),
    ('tn', 'gemm_tn_scaled', 257, 4, 64, 0, (0, 0, 0), None, 5, (0, 0, 0), ('tn', 1, 4, 1, 1, 1, 0, 1), ('M % 32 != 0, M no multiple of rows_per_slice', 'N % 32 != 0', 'K % 64 == 0', 'gate rows not dividing 16')),
    ('tn', 'gemm_tn_scaled', 257, 4, 60, 0, (0, 0, 0), None, 5, (0, 0, 0), ('tn', 1, 4, 1, 1, 1, 0, 1), ('M % 32 != 0, M no multiple of rows_per_slice', 'N % 32 != 0', 'K % 64 == 60', 'gate rows not dividing 16')),
    ('tn', 'gemm_tn_scaled', 257, 4, 4, 0, (0, 0, 0), None, 5, (0, 0, 0), ('tn', 1, 4, 1, 1, 1, 0, 1), ('M % 32 != 0, M no multiple of rows_per_slice', 'N % 32 != 0', 'K % 64 neither 0 nor 60', 'gate rows not dividing 16')),
    ('tn', 'gemm_tn_scaled', 6657, 252, 256, 0, (0, 0, 0), None, 5, (0, 0, 0), ('tn', 1, 4, 1, 1, 1, 0, 2), ('M % 32 != 0, M no multiple of rows_per_slice', 'an empty trailing slice', 'N % 32 != 0', 'K % 64 == 0', 'gate rows not dividing 16')),
    ('tn', 'gemm_tn_scaled', 8193, 252, 252, 0, (0, 0, 0), None, 5, (0, 0, 0), ('tn', 1, 4, 1, 1, 1, 0, 2), ('M % 32 != 0, M no multiple of rows_per_slice', 'an empty trailing slice', 'N % 32 != 0', 'K % 64 == 60', 'gate rows not dividing 16')),
    ('tn', 'gemm_tn_scaled', 6657, 252, 260, 0, (0, 0, 0), None, 5, (0, 0, 0), ('tn', 1, 4, 1, 1, 1, 0, 2), ('M % 32 != 0, M no multiple of rows_per_slice', 'an empty trailing slice', 'N % 32 != 0', 'K % 64 neither 0 nor 60', 'gate rows not dividing 16')),
    ('tn', 'gemm_tn_levels', 341, 256, 4, 2, (0, 87978, 258), (1, ((16, 16), (8, 8), (4, 4), (2, 2), (1, 1))), 0, (0, 0, 0), ('tn', 2, 2, 1, 0, 0, 2, 1), ()),
    ('tn', 'gemm_tn_levels', 341, 258, 64, 2, (0, 87978, 258), (1, ((16, 16), (8, 8), (4, 4), (2, 2), (1, 1))), 0, (0, 0, 0), ('tn', 2, 2, 1, 0, 0, 2, 1), ('M % 32 != 0, M no multiple of rows_per_slice', 'N % 128 != 0', 'K % 64 == 0')),
    ('tn', 'gemm_tn_levels', 341, 258, 60, 2, (0, 87978, 258), (1, ((16, 16), (8, 8), (4, 4), (2, 2), (1, 1))), 0, (0, 0, 0), ('tn', 2, 2, 1, 0, 0, 2, 1), ('M % 32 != 0, M no multiple of rows_per_slice', 'N % 128 != 0', 'K % 64 == 60')),
    ('tn', 'gemm_tn_levels', 341, 258, 4, 2, (0, 87978, 258), (1, ((16, 16), (8, 8), (4, 4), (2, 2), (1, 1))), 0, (0, 0, 0), ('tn', 2, 2, 1, 0, 0, 2, 1), ('M % 32 != 0, M no multiple of rows_per_slice', 'N % 128 != 0', 'K % 64 neither 0 nor 60')),
    ('tn', 'gemm_tn_levels', 5433, 544, 576, 2, (0, 988806, 546), (3, ((44, 41), (3, 2), (1, 1))), 0, (0, 0, 0), ('tn', 2, 2, 1, 0, 0, 2, 2), ('M % 32 != 0, M no multiple of rows_per_slice', 'an empty trailing slice', 'N % 128 != 0', 'K % 64 == 0')),
    ('tn', 'gemm_tn_levels', 6011, 544, 572, 2, (0, 3282006, 546), (1, ((79, 76), (3, 2), (1, 1))), 0, (0, 0, 0), ('tn', 2, 2, 1, 0, 0, 2, 2), ('M % 32 != 0, M no multiple of rows_per_slice', 'an empty trailing slice', 'N % 128 != 0', 'K % 64 == 60')),
    ('tn', 'gemm_tn_levels', 5433, 544, 580, 2, (0, 988806, 546), (3, ((44, 41), (3, 2), (1, 1))), 0, (0, 0, 0), ('tn', 2, 2, 1, 0, 0, 2, 2), ('M % 32 != 0, M no multiple of rows_per_slice', 'an empty trailing slice', 'N % 128 != 0', 'K % 64 neither 0 nor 60')),
    ('tn', 'gemm_tn', 1, 256, 4, 0, (0, 0, 0), None, 0, (0, 0, 0), ('tn', 2, 4, 1, 1, 0, 0, 0), ()),
    ('tn', 'gemm_tn', 1, 260, 64, 0, (0, 0, 0), None, 0, (0, 0, 0), ('tn', 2, 4, 1, 1, 0, 0, 0), ('M % 32 != 0, M no multiple of rows_per_slice', 'N % 128 != 0', 'K % 64 == 0')),
    ('tn', 'gemm_tn', 1, 260, 60, 0, (0, 0, 0), None, 0, (0, 0, 0), ('tn', 2, 4, 1, 1, 0, 0, 0), ('M % 32 != 0, M no multiple of rows_per_slice', 'N % 128 != 0', 'K % 64 == 60')),
    ('tn', 'gemm_tn', 1, 260, 4, 0, (0, 0, 0), None, 0, (0, 0, 0), ('tn', 2, 4, 1, 1, 0, 0, 0), ('M % 32 != 0, M no multiple of rows_per_slice', 'N % 128 != 0', 'K % 64 neither 0 nor 60')),
    ('tn', 'gemm_tn', 257, 256, 4, 0, (0, 0, 0), None, 0, (0, 0, 0), ('tn', 2, 4, 1, 1, 0, 0, 1), ()),
    ('tn', 'gemm_tn', 257, 260, 64, 0, (0, 0, 0), None, 0, (0, 0, 0), ('tn', 2, 4, 1, 1, 0, 0, 1), ('M % 32 != 0, M no multiple of rows_per_slice', 'N % 128 != 0', 'K % 64 == 0')),
    ('tn', 'gemm_tn', 257, 260, 60, 0, (0, 0, 0), None, 0, (0, 0, 0), ('tn', 2, 4, 1, 1, 0, 0, 1), ('M % 32 != 0, M no multiple of rows_per_slice', 'N % 128 != 0', 'K % 64 == 60')),
    ('tn', 'gemm_tn', 257, 260, 4, 0, (0, 0, 0), None, 0, (0, 0, 0), ('tn', 2, 4, 1, 1, 0, 0, 1), ('M % 32 != 0, M no multiple of rows_per_slice', 'N % 128 != 0', 'K % 64 neither 0 nor 60')),
    ('tn', 'gemm_tn', 5377, 544, 576, 0, (0, 0, 0), None, 0, (0, 0, 0), ('tn', 2, 4, 1, 1, 0, 0, 2), ('M % 32 != 0, M no multiple of rows_per_slice', 'an empty trailing slice', 'N % 128 != 0', 'K % 64 == 0')),
    ('tn', 'gemm_tn', 5889, 544, 572, 0, (0, 0, 0), None, 0, (0, 0, 0), ('tn', 2, 4, 1, 1, 0, 0, 2), ('M % 32 != 0, M no multiple of rows_per_slice', 'an empty trailing slice', 'N % 128 != 0', 'K % 64 == 60')),
    ('tn', 'gemm_tn', 5377, 544, 580, 0, (0, 0, 0), None, 0, (0, 0, 0), ('tn', 2, 4, 1, 1, 0, 0, 2), ('M % 32 != 0, M no multiple of rows_per_slice', 'an empty trailing slice', 'N % 128 != 0', 'K % 64 neither 0 nor 60')),
]
# fmt: on
# CASES-END
