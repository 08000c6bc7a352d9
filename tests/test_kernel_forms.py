"""Host-side form decisions of the fused MBConv and stem kernels (no GPU): the pool-partial row counts that the engine sizes its
buffers by and hands to the SE gate, swept over every backbone block, against tests/golden/kernel_forms.json."""
import ctypes
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = ['tf_efficientdet_d%d' % i for i in range(6)] + ['efficientdet_d%d' % i for i in range(6)]
SIZES = (512, 640, 768, 1024, 1280)
PAD = 1 << 24                                 # EFFDET_PAD_SYMMETRIC


def _same_out(n, s):
    return (n + s - 1) // s


def kernel_forms(lib_path):
    """{model: {size: {dtype[+pad]: {'stem': parts, 'tiles': [per ir block], 'gated': [per ir block]}}}} from the library at lib_path"""
    from ood_object_detection_amd.backbone import efficientnet_arch
    from ood_object_detection_amd.effdet.config import get_efficientdet_config
    import torch  # noqa: F401  (share torch's HIP runtime, see _lib.load)
    lib = ctypes.CDLL(lib_path)
    for name in ('effdet_mbconv_tiles_per_image', 'effdet_mbconv_gated_tiles_per_image'):
        getattr(lib, name).argtypes = [ctypes.c_int] * 7
    lib.effdet_stem_dw_parts.argtypes = [ctypes.c_int] * 4
    table = {}
    for model in MODELS:
        cfg = get_efficientdet_config(model)
        stem_c, stages = efficientnet_arch(cfg.backbone_name)
        for size in sorted({cfg.image_size[0]} | set(SIZES)):
            for dt in (0, 1, 2):
                for pad in (0, PAD):
                    h = w = _same_out(size, 2)
                    tiles, gated = [], []
                    for blocks in stages:
                        for b in blocks:
                            if b['type'] == 'ir':
                                args = (dt | pad, h, w, b['cin'], b['mid'], b['k'], b['s'])
                                tiles.append(lib.effdet_mbconv_tiles_per_image(*args))
                                gated.append(lib.effdet_mbconv_gated_tiles_per_image(*args))
                            h, w = _same_out(h, b['s']), _same_out(w, b['s'])
                    entry = dict(stem=lib.effdet_stem_dw_parts(dt | pad, size, size, stem_c), tiles=tiles, gated=gated)
                    table.setdefault(model, {}).setdefault(str(size), {})['%d%s' % (dt, '+pad' if pad else '')] = entry
    return table


def test_kernel_forms_match_golden():
    """every fused-form query answers as recorded (a changed count means a changed kernel form or pool-partial layout)"""
    from ood_object_detection_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    with open(os.path.join(ROOT, 'tests', 'golden', 'kernel_forms.json')) as f:
        ref = json.load(f)
    got = kernel_forms(_lib.LIB_PATH)
    assert sorted(got) == sorted(ref)
    for model in ref:
        for size in ref[model]:
            for dt in ref[model][size]:
                assert got[model][size][dt] == ref[model][size][dt], (model, size, dt)
