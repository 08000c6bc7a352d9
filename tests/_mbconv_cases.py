"""Case table of tests/test_mbconv_variants_{host,gpu}.py: one small problem per fused-MBConv kernel variant that the d0 ... d5
backbones run, plus the edge geometries of every (dtype, form).  No GPU code here: the plan of a case is asked of the library's
host-only query effdet_mbconv_plan_describe, which is answered by the launcher's own mbconv_plan().

A case is (dtype, gated, Cin, mid, H, W, k, s, cls, edges): dtype 0 float32 / 1 bf16 / 2 two-term bf16, gated = the input is
multiplied by a per-image channel gate (effdet_mbconv_expand_dw_gated), edges the names of the edge geometries (EDGES) the case
is in the table for, and cls the class the case is meant to reach:
    cls = (dtype, gated, form, variant key)
    variant key   roll:  (pair, k, s, nkc, MT, NO, NJ)          wide:  (pair, k, s, nkc, MT, NO, NPL)
                  deep:  (T, k, s, lds > 78 KiB, lds > 64 KiB, nbands > 1, nchunks > 1)
                  front: (T, k, s, TH, TW, lds > 64 KiB)
CLASS_COUNTS and CASES are generated (the block between CASES-BEGIN and CASES-END): tools/make_mbconv_cases.py sweeps the backbones,
searches the cheapest problem of every class and of every edge geometry and rewrites that block in place
(tests/test_mbconv_variants_host.py fails when the table and the sweep disagree)."""
import ctypes

PAD = 1 << 24                                 # EFFDET_PAD_SYMMETRIC
NONE, ROLL, WIDE, DEEP, FRONT = 0, 1, 2, 3, 4
FORM_NAME = {NONE: 'none', ROLL: 'roll', WIDE: 'wide', DEEP: 'deep', FRONT: 'front'}
DTYPE_NAME = {0: 'float32', 1: 'bf16', 2: 'two-term bf16'}
PLAN_INTS = 17
FIELDS = ('form', 'parts', 'nkc', 'MT', 'NO', 'NJ', 'TWo', 'nstrips', 'band_rows', 'nbands', 'waves', 'lds', 'nchunks',
          'TH', 'TW', 'tiles_x', 'tiles_y')          # slot order of effdet_mbconv_plan_describe ('NJ': NJ of roll / NPL of wide)
MODELS = ['tf_efficientdet_d%d' % i for i in range(6)]
SIZES = (128, 256, 384, 512, 640, 768, 1024, 1280)    # tests/test_kernel_forms.py's sizes and the small sizes the suite and smoke() run
                                                        # (128, 256, 384); each model's native size is added
MAX_ELEMS = 4e6                               # B * Ho * Wo * mid of a case
B = 2                                         # images of a case in the GPU test


SMALLEST = 4                                  # the smallest map of the sweep (128 px / 32): floor of the cases no larger map serves


def floor(k):
    """smallest H and W of a case: one output pixel whose whole window lies inside the map, next to both borders"""
    return 2 * k + 1


def same_out(n, s):
    return (n + s - 1) // s


def plan(lib, dtype, gated, Cin, mid, H, W, k, s):
    """the library's plan of one block as a dict over FIELDS"""
    out = (ctypes.c_int * PLAN_INTS)()
    n = lib.effdet_mbconv_plan_describe(dtype, H, W, Cin, mid, k, s, int(gated), out, PLAN_INTS)
    assert n == PLAN_INTS, n
    return dict(zip(FIELDS, out))


def variant_key(p, dtype, k, s):
    f = p['form']
    if f in (ROLL, WIDE):
        return (int(dtype == 2), k, s, p['nkc'], p['MT'], p['NO'], p['NJ'])
    if f == DEEP:
        return (dtype, k, s, p['lds'] > 78 * 1024, p['lds'] > 64 * 1024, p['nbands'] > 1, p['nchunks'] > 1)
    if f == FRONT:
        return (dtype, k, s, p['TH'], p['TW'], p['lds'] > 64 * 1024)
    return ()


def klass(p, dtype, gated, k, s):
    return (dtype, int(gated), p['form'], variant_key(p, dtype, k, s))


def case_plan(lib, case):
    dtype, gated, Cin, mid, H, W, k, s = case[:8]
    return plan(lib, dtype, gated, Cin, mid, H, W, k, s)


def case_class(lib, case):
    dtype, gated, Cin, mid, H, W, k, s = case[:8]
    return klass(case_plan(lib, case), dtype, gated, k, s)


def case_id(case):
    dtype, gated, Cin, mid, H, W, k, s = case[:8]
    return '%s%s-%s-c%d-m%d-%dx%d-k%ds%d' % (('f32', 'bf16', 'pair')[dtype], '-gated' if gated else '', FORM_NAME[case[8][2]], Cin, mid, H, W, k, s)


def swept_blocks():
    """(model, size, dtype, gated, Cin, mid, H, W, k, s) of every inverted-residual block of d0 ... d5 at SIZES and the native size,
    dtypes 0 / 1 / 2.  The first ir block also runs gated: the engine composes block 0.0's project conv into its expand weights,
    so its gated input has block 0.0's mid channels (engine.Engine._build_backbone); its own Cin is swept gated too, as
    tests/test_kernel_forms.py does."""
    from ood_object_detection_amd.backbone import efficientnet_arch
    from ood_object_detection_amd.effdet.config import get_efficientdet_config
    out = []
    for model in MODELS:
        cfg = get_efficientdet_config(model)
        stem_c, stages = efficientnet_arch(cfg.backbone_name)
        for size in sorted({cfg.image_size[0]} | set(SIZES)):
            h = w = same_out(size, 2)
            first, prev_mid = True, None
            for blocks in stages:
                for b in blocks:
                    if b['type'] == 'ir':
                        for dt in (0, 1, 2):
                            out.append((model, size, dt, 0, b['cin'], b['mid'], h, w, b['k'], b['s']))
                            if first:
                                for cin in sorted({b['cin'], prev_mid or b['cin']}):
                                    out.append((model, size, dt, 1, cin, b['mid'], h, w, b['k'], b['s']))
                        first = False
                    prev_mid = b['mid']
                    h, w = same_out(h, b['s']), same_out(w, b['s'])
    return out


def used_classes(lib):
    """{class: first swept block that has it} over swept_blocks(), form 'none' left out"""
    used = {}
    for blk in swept_blocks():
        dt, gated, Cin, mid, H, W, k, s = blk[2:]
        c = klass(plan(lib, dt, gated, Cin, mid, H, W, k, s), dt, gated, k, s)
        if c[2] != NONE:
            used.setdefault(c, blk)
    return used


# ---- edge geometries: (name, applies(form, s), holds(plan, case)) - asserted per (dtype, form) by the host test
def _ragged_cols(p, case):
    Wo = same_out(case[5], case[7])
    if p['form'] in (ROLL, WIDE):
        return p['nstrips'] > 1 and Wo % p['TWo'] != 0
    return p['form'] == FRONT and p['tiles_x'] > 1 and Wo % p['TW'] != 0


def _ragged_rows(p, case):
    Ho = same_out(case[4], case[7])
    if p['form'] == FRONT:
        return p['tiles_y'] > 1 and Ho % p['TH'] != 0
    return p['nbands'] > 1 and Ho % p['band_rows'] != 0


EDGES = (
    ('ragged last strip / tile column', lambda form: form != DEEP, _ragged_cols),     # (the deep form's bands span whole rows)
    ('ragged last band / tile row', lambda form: True, _ragged_rows),
    ('odd H and odd W', lambda form: True, lambda p, c: c[4] % 2 == 1 and c[5] % 2 == 1),
    ('stride 2, even map', lambda form: True, lambda p, c: c[7] == 2 and c[4] % 2 == 0 and c[5] % 2 == 0),
    ('stride 2, odd map', lambda form: True, lambda p, c: c[7] == 2 and c[4] % 2 == 1 and c[5] % 2 == 1),
)

# CASES-BEGIN
# classes per (dtype, form) that the sweep of swept_blocks() finds (recorded in DESIGN.md; the host test recounts them)
CLASS_COUNTS = {(0, DEEP): 18, (0, FRONT): 16, (1, ROLL): 28, (1, WIDE): 30, (1, DEEP): 14, (1, FRONT): 3, (2, ROLL): 18, (2, WIDE): 36}

# fmt: off
CASES = [
    (0, 0, 80, 480, 7, 7, 3, 1, (0, 0, 3, (0, 3, 1, False, False, False, True)), ()),
    (0, 0, 80, 480, 12, 18, 3, 1, (0, 0, 3, (0, 3, 1, False, False, True, True)), ()),
    (0, 0, 208, 1248, 7, 7, 3, 1, (0, 0, 3, (0, 3, 1, False, True, False, True)), ()),
    (0, 0, 32, 192, 7, 38, 3, 1, (0, 0, 3, (0, 3, 1, False, True, True, True)), ()),
    (0, 0, 272, 1632, 7, 7, 3, 1, (0, 0, 3, (0, 3, 1, True, True, False, True)), ()),
    (0, 0, 512, 3072, 8, 13, 3, 1, (0, 0, 3, (0, 3, 1, True, True, True, True)), ()),
    (0, 0, 40, 240, 14, 18, 3, 2, (0, 0, 3, (0, 3, 2, False, False, True, True)), ()),
    (0, 0, 40, 240, 9, 28, 3, 2, (0, 0, 3, (0, 3, 2, False, True, True, True)), ()),
    (0, 0, 80, 480, 11, 11, 5, 1, (0, 0, 3, (0, 5, 1, False, False, False, True)), ()),
    (0, 0, 40, 240, 19, 13, 5, 1, (0, 0, 3, (0, 5, 1, False, False, True, True)), ()),
    (0, 0, 232, 1392, 4, 4, 5, 1, (0, 0, 3, (0, 5, 1, False, True, False, True)), ()),
    (0, 0, 40, 240, 13, 19, 5, 1, (0, 0, 3, (0, 5, 1, False, True, True, True)), ()),
    (0, 0, 232, 1392, 11, 11, 5, 1, (0, 0, 3, (0, 5, 1, True, True, False, True)), ()),
    (0, 0, 128, 768, 16, 29, 5, 1, (0, 0, 3, (0, 5, 1, True, True, True, True)), ()),
    (0, 0, 112, 672, 11, 11, 5, 2, (0, 0, 3, (0, 5, 2, False, False, False, True)), ()),
    (0, 0, 112, 672, 12, 16, 5, 2, (0, 0, 3, (0, 5, 2, False, True, True, True)), ()),
    (0, 0, 176, 1056, 11, 14, 5, 2, (0, 0, 3, (0, 5, 2, True, True, False, True)), ()),
    (0, 0, 136, 816, 12, 38, 5, 2, (0, 0, 3, (0, 5, 2, True, True, True, True)), ()),
    (0, 0, 80, 480, 7, 43, 3, 1, (0, 0, 4, (0, 3, 1, 4, 8, False)), ()),
    (0, 0, 96, 576, 7, 40, 3, 1, (0, 0, 4, (0, 3, 1, 4, 8, True)), ()),
    (0, 0, 40, 240, 8, 49, 3, 1, (0, 0, 4, (0, 3, 1, 8, 8, False)), ()),
    (0, 0, 24, 144, 8, 8, 3, 1, (0, 0, 4, (0, 3, 1, 8, 16, True)), ()),
    (0, 0, 56, 336, 8, 29, 3, 2, (0, 0, 4, (0, 3, 2, 4, 4, False)), ()),
    (0, 0, 16, 96, 7, 7, 3, 2, (0, 0, 4, (0, 3, 2, 4, 8, False)), ()),
    (0, 0, 40, 240, 8, 31, 3, 2, (0, 0, 4, (0, 3, 2, 4, 8, True)), ()),
    (0, 0, 128, 768, 11, 67, 5, 1, (0, 0, 4, (0, 5, 1, 2, 4, True)), ()),
    (0, 0, 96, 576, 11, 29, 5, 1, (0, 0, 4, (0, 5, 1, 4, 4, True)), ()),
    (0, 0, 56, 336, 11, 33, 5, 1, (0, 0, 4, (0, 5, 1, 4, 8, False)), ()),
    (0, 0, 80, 480, 11, 31, 5, 1, (0, 0, 4, (0, 5, 1, 4, 8, True)), ()),
    (0, 0, 40, 240, 11, 35, 5, 1, (0, 0, 4, (0, 5, 1, 8, 8, True)), ()),
    (0, 0, 120, 720, 11, 19, 5, 2, (0, 0, 4, (0, 5, 2, 2, 4, True)), ()),
    (0, 0, 24, 144, 11, 11, 5, 2, (0, 0, 4, (0, 5, 2, 4, 4, False)), ()),
    (0, 1, 16, 96, 7, 7, 3, 2, (0, 1, 4, (0, 3, 2, 4, 8, False)), ()),
    (0, 1, 32, 96, 7, 7, 3, 2, (0, 1, 4, (0, 3, 2, 4, 8, True)), ()),
    (1, 0, 24, 144, 7, 31, 3, 1, (1, 0, 1, (0, 3, 1, 1, 3, 2, 1)), ()),
    (1, 0, 24, 144, 7, 33, 3, 1, (1, 0, 1, (0, 3, 1, 1, 3, 3, 1)), ()),
    (1, 0, 24, 144, 7, 47, 3, 1, (1, 0, 1, (0, 3, 1, 1, 4, 3, 1)), ()),
    (1, 0, 24, 144, 7, 49, 3, 1, (1, 0, 1, (0, 3, 1, 1, 4, 4, 1)), ()),
    (1, 0, 40, 240, 7, 31, 3, 1, (1, 0, 1, (0, 3, 1, 2, 3, 2, 1)), ()),
    (1, 0, 40, 240, 7, 33, 3, 1, (1, 0, 1, (0, 3, 1, 2, 3, 3, 1)), ()),
    (1, 0, 40, 240, 7, 47, 3, 1, (1, 0, 1, (0, 3, 1, 2, 4, 3, 1)), ()),
    (1, 0, 40, 240, 7, 49, 3, 1, (1, 0, 1, (0, 3, 1, 2, 4, 4, 1)), ()),
    (1, 0, 16, 96, 7, 7, 3, 2, (1, 0, 1, (0, 3, 2, 1, 2, 1, 1)), ()),
    (1, 0, 16, 96, 7, 31, 3, 2, (1, 0, 1, (0, 3, 2, 1, 3, 1, 1)), ()),
    (1, 0, 16, 96, 7, 33, 3, 2, (1, 0, 1, (0, 3, 2, 1, 3, 2, 1)), ()),
    (1, 0, 16, 96, 7, 47, 3, 2, (1, 0, 1, (0, 3, 2, 1, 4, 2, 1)), ()),
    (1, 0, 40, 240, 7, 7, 3, 2, (1, 0, 1, (0, 3, 2, 2, 2, 1, 1)), ()),
    (1, 0, 40, 240, 11, 11, 5, 1, (1, 0, 1, (0, 5, 1, 2, 2, 1, 1)), ()),
    (1, 0, 48, 288, 11, 17, 5, 1, (1, 0, 1, (0, 5, 1, 2, 2, 2, 1)), ()),
    (1, 0, 40, 240, 11, 29, 5, 1, (1, 0, 1, (0, 5, 1, 2, 3, 2, 1)), ()),
    (1, 0, 40, 240, 11, 33, 5, 1, (1, 0, 1, (0, 5, 1, 2, 3, 3, 1)), ()),
    (1, 0, 24, 144, 11, 11, 5, 2, (1, 0, 1, (0, 5, 2, 1, 2, 1, 1)), ()),
    (1, 0, 24, 144, 11, 29, 5, 2, (1, 0, 1, (0, 5, 2, 1, 3, 1, 1)), ()),
    (1, 0, 40, 240, 11, 11, 5, 2, (1, 0, 1, (0, 5, 2, 2, 2, 1, 1)), ()),
    (1, 0, 80, 480, 7, 24, 3, 1, (1, 0, 2, (0, 3, 1, 3, 2, 2, 1)), ()),
    (1, 0, 80, 480, 7, 31, 3, 1, (1, 0, 2, (0, 3, 1, 3, 3, 2, 1)), ()),
    (1, 0, 80, 480, 7, 36, 3, 1, (1, 0, 2, (0, 3, 1, 3, 3, 3, 1)), ()),
    (1, 0, 80, 480, 7, 47, 3, 1, (1, 0, 2, (0, 3, 1, 3, 4, 3, 1)), ()),
    (1, 0, 96, 576, 7, 49, 3, 1, (1, 0, 2, (0, 3, 1, 3, 4, 4, 1)), ()),
    (1, 0, 112, 672, 7, 24, 3, 1, (1, 0, 2, (0, 3, 1, 4, 2, 2, 1)), ()),
    (1, 0, 112, 672, 7, 31, 3, 1, (1, 0, 2, (0, 3, 1, 4, 3, 2, 1)), ()),
    (1, 0, 112, 672, 7, 36, 3, 1, (1, 0, 2, (0, 3, 1, 4, 3, 3, 1)), ()),
    (1, 0, 112, 672, 7, 47, 3, 1, (1, 0, 2, (0, 3, 1, 4, 4, 3, 1)), ()),
    (1, 0, 192, 1152, 7, 24, 3, 1, (1, 0, 2, (0, 3, 1, 6, 2, 2, 1)), ()),
    (1, 0, 80, 480, 11, 16, 5, 1, (1, 0, 2, (0, 5, 1, 3, 2, 1, 1)), ()),
    (1, 0, 80, 480, 11, 23, 5, 1, (1, 0, 2, (0, 5, 1, 3, 2, 2, 1)), ()),
    (1, 0, 80, 480, 11, 29, 5, 1, (1, 0, 2, (0, 5, 1, 3, 3, 2, 1)), ()),
    (1, 0, 80, 480, 11, 35, 5, 1, (1, 0, 2, (0, 5, 1, 3, 3, 3, 1)), ()),
    (1, 0, 112, 672, 11, 16, 5, 1, (1, 0, 2, (0, 5, 1, 4, 2, 1, 1)), ()),
    (1, 0, 112, 672, 11, 23, 5, 1, (1, 0, 2, (0, 5, 1, 4, 2, 2, 1)), ()),
    (1, 0, 112, 672, 11, 29, 5, 1, (1, 0, 2, (0, 5, 1, 4, 3, 2, 1)), ()),
    (1, 0, 112, 672, 11, 35, 5, 1, (1, 0, 2, (0, 5, 1, 4, 3, 3, 1)), ()),
    (1, 0, 160, 960, 11, 16, 5, 1, (1, 0, 2, (0, 5, 1, 5, 2, 1, 1)), ()),
    (1, 0, 160, 960, 11, 23, 5, 1, (1, 0, 2, (0, 5, 1, 5, 2, 2, 1)), ()),
    (1, 0, 160, 960, 11, 29, 5, 1, (1, 0, 2, (0, 5, 1, 5, 3, 2, 1)), ()),
    (1, 0, 160, 960, 11, 35, 5, 1, (1, 0, 2, (0, 5, 1, 5, 3, 3, 1)), ()),
    (1, 0, 176, 1056, 11, 16, 5, 1, (1, 0, 2, (0, 5, 1, 6, 2, 1, 1)), ()),
    (1, 0, 176, 1056, 11, 23, 5, 1, (1, 0, 2, (0, 5, 1, 6, 2, 2, 1)), ()),
    (1, 0, 112, 672, 11, 21, 5, 2, (1, 0, 2, (0, 5, 2, 4, 2, 1, 1)), ()),
    (1, 0, 112, 672, 11, 31, 5, 2, (1, 0, 2, (0, 5, 2, 4, 3, 1, 1)), ()),
    (1, 0, 112, 672, 11, 37, 5, 2, (1, 0, 2, (0, 5, 2, 4, 3, 2, 1)), ()),
    (1, 0, 160, 960, 11, 21, 5, 2, (1, 0, 2, (0, 5, 2, 5, 2, 1, 1)), ()),
    (1, 0, 160, 960, 11, 31, 5, 2, (1, 0, 2, (0, 5, 2, 5, 3, 1, 1)), ()),
    (1, 0, 176, 1056, 11, 21, 5, 2, (1, 0, 2, (0, 5, 2, 6, 2, 1, 1)), ()),
    (1, 0, 80, 480, 7, 7, 3, 1, (1, 0, 3, (1, 3, 1, False, False, False, True)), ()),
    (1, 0, 192, 1152, 7, 40, 3, 1, (1, 0, 3, (1, 3, 1, False, False, True, True)), ()),
    (1, 0, 448, 2688, 7, 7, 3, 1, (1, 0, 3, (1, 3, 1, False, True, False, True)), ()),
    (1, 0, 512, 3072, 7, 9, 3, 1, (1, 0, 3, (1, 3, 1, False, True, True, True)), ()),
    (1, 0, 512, 3072, 7, 17, 3, 1, (1, 0, 3, (1, 3, 1, True, True, False, True)), ()),
    (1, 0, 384, 2304, 7, 83, 3, 1, (1, 0, 3, (1, 3, 1, True, True, True, True)), ()),
    (1, 0, 80, 480, 11, 11, 5, 1, (1, 0, 3, (1, 5, 1, False, False, False, True)), ()),
    (1, 0, 208, 1248, 12, 18, 5, 1, (1, 0, 3, (1, 5, 1, False, False, True, True)), ()),
    (1, 0, 136, 816, 13, 14, 5, 1, (1, 0, 3, (1, 5, 1, False, True, False, True)), ()),
    (1, 0, 136, 816, 11, 27, 5, 1, (1, 0, 3, (1, 5, 1, False, True, True, True)), ()),
    (1, 0, 272, 1632, 11, 53, 5, 1, (1, 0, 3, (1, 5, 1, True, True, True, True)), ()),
    (1, 0, 112, 672, 11, 11, 5, 2, (1, 0, 3, (1, 5, 2, False, False, False, True)), ()),
    (1, 0, 112, 672, 11, 19, 5, 2, (1, 0, 3, (1, 5, 2, False, True, False, True)), ()),
    (1, 0, 136, 816, 13, 25, 5, 2, (1, 0, 3, (1, 5, 2, False, True, True, True)), ()),
    (1, 0, 136, 816, 11, 54, 5, 1, (1, 0, 4, (1, 5, 1, 4, 8, True)), ()),
    (1, 0, 176, 1056, 11, 39, 5, 2, (1, 0, 4, (1, 5, 2, 2, 4, True)), ()),
    (1, 0, 136, 816, 11, 43, 5, 2, (1, 0, 4, (1, 5, 2, 4, 4, True)), ()),
    (1, 1, 16, 96, 7, 7, 3, 2, (1, 1, 1, (0, 3, 2, 1, 2, 1, 1)), ()),
    (1, 1, 32, 96, 7, 7, 3, 2, (1, 1, 1, (0, 3, 2, 1, 2, 1, 2)), ()),
    (1, 1, 16, 96, 7, 31, 3, 2, (1, 1, 1, (0, 3, 2, 1, 3, 1, 1)), ()),
    (1, 1, 32, 96, 7, 31, 3, 2, (1, 1, 1, (0, 3, 2, 1, 3, 1, 2)), ()),
    (1, 1, 16, 96, 7, 33, 3, 2, (1, 1, 1, (0, 3, 2, 1, 3, 2, 1)), ()),
    (1, 1, 32, 96, 7, 33, 3, 2, (1, 1, 1, (0, 3, 2, 1, 3, 2, 2)), ()),
    (1, 1, 16, 96, 7, 47, 3, 2, (1, 1, 1, (0, 3, 2, 1, 4, 2, 1)), ()),
    (1, 1, 32, 96, 7, 47, 3, 2, (1, 1, 1, (0, 3, 2, 1, 4, 2, 2)), ()),
    (2, 0, 24, 144, 7, 17, 3, 1, (2, 0, 1, (1, 3, 1, 1, 2, 2, 2)), ()),
    (2, 0, 24, 144, 7, 31, 3, 1, (2, 0, 1, (1, 3, 1, 1, 3, 2, 2)), ()),
    (2, 0, 24, 144, 7, 33, 3, 1, (2, 0, 1, (1, 3, 1, 1, 3, 3, 2)), ()),
    (2, 0, 40, 240, 7, 17, 3, 1, (2, 0, 1, (1, 3, 1, 2, 2, 2, 1)), ()),
    (2, 0, 40, 240, 7, 31, 3, 1, (2, 0, 1, (1, 3, 1, 2, 3, 2, 1)), ()),
    (2, 0, 40, 240, 7, 33, 3, 1, (2, 0, 1, (1, 3, 1, 2, 3, 3, 1)), ()),
    (2, 0, 16, 96, 7, 7, 3, 2, (2, 0, 1, (1, 3, 2, 1, 2, 1, 2)), ()),
    (2, 0, 16, 96, 7, 31, 3, 2, (2, 0, 1, (1, 3, 2, 1, 3, 1, 2)), ()),
    (2, 0, 16, 96, 7, 33, 3, 2, (2, 0, 1, (1, 3, 2, 1, 3, 2, 2)), ()),
    (2, 0, 40, 240, 7, 7, 3, 2, (2, 0, 1, (1, 3, 2, 2, 2, 1, 1)), ()),
    (2, 0, 40, 240, 11, 11, 5, 1, (2, 0, 1, (1, 5, 1, 2, 2, 1, 1)), ()),
    (2, 0, 40, 240, 11, 17, 5, 1, (2, 0, 1, (1, 5, 1, 2, 2, 2, 1)), ()),
    (2, 0, 24, 144, 11, 11, 5, 2, (2, 0, 1, (1, 5, 2, 1, 2, 1, 1)), ()),
    (2, 0, 24, 144, 11, 29, 5, 2, (2, 0, 1, (1, 5, 2, 1, 3, 1, 1)), ()),
    (2, 0, 40, 240, 11, 11, 5, 2, (2, 0, 1, (1, 5, 2, 2, 2, 1, 1)), ()),
    (2, 0, 96, 576, 7, 15, 3, 1, (2, 0, 2, (1, 3, 1, 3, 2, 1, 2)), ()),
    (2, 0, 80, 480, 7, 15, 3, 1, (2, 0, 2, (1, 3, 1, 3, 2, 1, 3)), ()),
    (2, 0, 80, 480, 7, 24, 3, 1, (2, 0, 2, (1, 3, 1, 3, 2, 2, 2)), ()),
    (2, 0, 88, 528, 7, 17, 3, 1, (2, 0, 2, (1, 3, 1, 3, 2, 2, 3)), ()),
    (2, 0, 80, 480, 7, 18, 3, 1, (2, 0, 2, (1, 3, 1, 3, 2, 2, 4)), ()),
    (2, 0, 112, 672, 7, 15, 3, 1, (2, 0, 2, (1, 3, 1, 4, 2, 1, 2)), ()),
    (2, 0, 112, 672, 9, 15, 3, 1, (2, 0, 2, (1, 3, 1, 4, 2, 1, 4)), ()),
    (2, 0, 112, 672, 7, 17, 3, 1, (2, 0, 2, (1, 3, 1, 4, 2, 2, 2)), ()),
    (2, 0, 192, 1152, 7, 15, 3, 1, (2, 0, 2, (1, 3, 1, 6, 2, 1, 2)), ()),
    (2, 0, 192, 1152, 7, 20, 3, 1, (2, 0, 2, (1, 3, 1, 6, 2, 2, 3)), ()),
    (2, 0, 96, 576, 11, 13, 5, 1, (2, 0, 2, (1, 5, 1, 3, 2, 1, 2)), ()),
    (2, 0, 88, 528, 11, 14, 5, 1, (2, 0, 2, (1, 5, 1, 3, 2, 1, 3)), ()),
    (2, 0, 80, 480, 11, 16, 5, 1, (2, 0, 2, (1, 5, 1, 3, 2, 1, 4)), ()),
    (2, 0, 80, 480, 11, 22, 5, 1, (2, 0, 2, (1, 5, 1, 3, 2, 2, 2)), ()),
    (2, 0, 88, 528, 11, 17, 5, 1, (2, 0, 2, (1, 5, 1, 3, 2, 2, 3)), ()),
    (2, 0, 80, 480, 11, 17, 5, 1, (2, 0, 2, (1, 5, 1, 3, 2, 2, 4)), ()),
    (2, 0, 112, 672, 11, 13, 5, 1, (2, 0, 2, (1, 5, 1, 4, 2, 1, 2)), ()),
    (2, 0, 120, 720, 11, 16, 5, 1, (2, 0, 2, (1, 5, 1, 4, 2, 1, 4)), ()),
    (2, 0, 112, 672, 11, 17, 5, 1, (2, 0, 2, (1, 5, 1, 4, 2, 2, 2)), ()),
    (2, 0, 120, 720, 11, 22, 5, 1, (2, 0, 2, (1, 5, 1, 4, 2, 2, 3)), ()),
    (2, 0, 120, 720, 11, 17, 5, 1, (2, 0, 2, (1, 5, 1, 4, 2, 2, 4)), ()),
    (2, 0, 136, 816, 11, 13, 5, 1, (2, 0, 2, (1, 5, 1, 5, 2, 1, 4)), ()),
    (2, 0, 160, 960, 11, 22, 5, 1, (2, 0, 2, (1, 5, 1, 5, 2, 2, 3)), ()),
    (2, 0, 160, 960, 11, 17, 5, 1, (2, 0, 2, (1, 5, 1, 5, 2, 2, 4)), ()),
    (2, 0, 192, 1152, 11, 13, 5, 1, (2, 0, 2, (1, 5, 1, 6, 2, 1, 2)), ()),
    (2, 0, 176, 1056, 11, 14, 5, 1, (2, 0, 2, (1, 5, 1, 6, 2, 1, 3)), ()),
    (2, 0, 176, 1056, 11, 17, 5, 1, (2, 0, 2, (1, 5, 1, 6, 2, 2, 3)), ()),
    (2, 0, 176, 1056, 11, 23, 5, 1, (2, 0, 2, (1, 5, 1, 6, 2, 2, 4)), ()),
    (2, 0, 112, 672, 11, 13, 5, 2, (2, 0, 2, (1, 5, 2, 4, 2, 1, 2)), ()),
    (2, 0, 120, 720, 11, 13, 5, 2, (2, 0, 2, (1, 5, 2, 4, 2, 1, 3)), ()),
    (2, 0, 120, 720, 11, 17, 5, 2, (2, 0, 2, (1, 5, 2, 4, 2, 1, 4)), ()),
    (2, 0, 160, 960, 11, 13, 5, 2, (2, 0, 2, (1, 5, 2, 5, 2, 1, 2)), ()),
    (2, 0, 160, 960, 11, 17, 5, 2, (2, 0, 2, (1, 5, 2, 5, 2, 1, 3)), ()),
    (2, 0, 136, 816, 11, 13, 5, 2, (2, 0, 2, (1, 5, 2, 5, 2, 1, 4)), ()),
    (2, 0, 176, 1056, 11, 15, 5, 2, (2, 0, 2, (1, 5, 2, 6, 2, 1, 3)), ()),
    (2, 0, 176, 1056, 11, 23, 5, 2, (2, 0, 2, (1, 5, 2, 6, 2, 1, 4)), ()),
    (2, 1, 16, 96, 7, 7, 3, 2, (2, 1, 1, (1, 3, 2, 1, 2, 1, 2)), ()),
    (2, 1, 16, 96, 7, 31, 3, 2, (2, 1, 1, (1, 3, 2, 1, 3, 1, 2)), ()),
    (2, 1, 16, 96, 7, 33, 3, 2, (2, 1, 1, (1, 3, 2, 1, 3, 2, 2)), ()),
    (0, 0, 40, 240, 13, 19, 3, 2, (0, 0, 3, (0, 3, 2, False, False, True, True)), ('ragged last band / tile row', 'odd H and odd W', 'stride 2, odd map')),
    (0, 0, 40, 240, 14, 18, 3, 2, (0, 0, 3, (0, 3, 2, False, False, True, True)), ('ragged last band / tile row', 'stride 2, even map')),
    (0, 0, 16, 96, 9, 17, 3, 2, (0, 0, 4, (0, 3, 2, 4, 8, False)), ('ragged last strip / tile column', 'ragged last band / tile row', 'odd H and odd W', 'stride 2, odd map')),
    (0, 0, 16, 96, 10, 18, 3, 2, (0, 0, 4, (0, 3, 2, 4, 8, False)), ('ragged last strip / tile column', 'ragged last band / tile row', 'stride 2, even map')),
    (1, 0, 16, 96, 161, 67, 3, 2, (1, 0, 1, (0, 3, 2, 1, 2, 1, 1)), ('ragged last strip / tile column', 'ragged last band / tile row', 'odd H and odd W', 'stride 2, odd map')),
    (1, 0, 16, 96, 162, 68, 3, 2, (1, 0, 1, (0, 3, 2, 1, 2, 1, 1)), ('ragged last strip / tile column', 'ragged last band / tile row', 'stride 2, even map')),
    (1, 0, 112, 672, 13, 61, 5, 2, (1, 0, 2, (0, 5, 2, 4, 3, 1, 1)), ('ragged last strip / tile column', 'ragged last band / tile row', 'odd H and odd W', 'stride 2, odd map')),
    (1, 0, 112, 672, 14, 62, 5, 2, (1, 0, 2, (0, 5, 2, 4, 3, 1, 1)), ('ragged last strip / tile column', 'ragged last band / tile row', 'stride 2, even map')),
    (1, 0, 112, 672, 25, 11, 5, 2, (1, 0, 3, (1, 5, 2, False, False, True, True)), ('ragged last band / tile row', 'odd H and odd W', 'stride 2, odd map')),
    (1, 0, 112, 672, 26, 12, 5, 2, (1, 0, 3, (1, 5, 2, False, False, True, True)), ('ragged last band / tile row', 'stride 2, even map')),
    (1, 0, 136, 816, 11, 43, 5, 2, (1, 0, 4, (1, 5, 2, 4, 4, True)), ('ragged last strip / tile column', 'ragged last band / tile row', 'odd H and odd W', 'stride 2, odd map')),
    (1, 0, 136, 816, 12, 44, 5, 2, (1, 0, 4, (1, 5, 2, 4, 4, True)), ('ragged last strip / tile column', 'ragged last band / tile row', 'stride 2, even map')),
    (2, 0, 16, 96, 161, 49, 3, 2, (2, 0, 1, (1, 3, 2, 1, 2, 1, 2)), ('ragged last strip / tile column', 'ragged last band / tile row', 'odd H and odd W', 'stride 2, odd map')),
    (2, 0, 16, 96, 162, 50, 3, 2, (2, 0, 1, (1, 3, 2, 1, 2, 1, 2)), ('ragged last strip / tile column', 'ragged last band / tile row', 'stride 2, even map')),
    (2, 0, 136, 816, 37, 29, 5, 2, (2, 0, 2, (1, 5, 2, 5, 2, 1, 4)), ('ragged last strip / tile column', 'ragged last band / tile row', 'odd H and odd W', 'stride 2, odd map')),
    (2, 0, 136, 816, 38, 30, 5, 2, (2, 0, 2, (1, 5, 2, 5, 2, 1, 4)), ('ragged last strip / tile column', 'ragged last band / tile row', 'stride 2, even map')),
]
# fmt: on
# CASES-END
