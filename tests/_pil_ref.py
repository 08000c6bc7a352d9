"""Test yardstick for the batched image / box transforms: a numpy restatement of Pillow's 8-bit BILINEAR and BICUBIC resample
(src/libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc, ImagingResampleHorizontal / Vertical_8bpc), of the
flip / crop / window / paste steps of effdet/data/transforms.py and of its box arithmetic.  tests/test_resample_host.py pins it
bit for bit against PIL itself and against the reference's recorded outputs (tests/golden/transforms.npz); the GPU tests
compare the kernels with it.  Scalar loops on purpose: every line is one line of the C source."""
import numpy as np

PRECISION_BITS = 32 - 8 - 2
BILINEAR, BICUBIC = 0, 1


def _bilinear(x):
    x = -x if x < 0.0 else x
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x):
    a = -0.5
    x = -x if x < 0.0 else x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def coeffs(in_size, out_size, filt):
    """-> (bounds int32 [out, 2] = (first source index, count), integer coefficients int32 [out, ksize])."""
    fn, sup = ((_bilinear, 1.0), (_bicubic, 2.0))[filt]
    scale = float(in_size) / out_size
    filterscale = max(scale, 1.0)
    support = sup * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [fn((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x in range(xmax):
            k = w[x] / ww if ww != 0.0 else w[x]
            kk[xx, x] = int(-0.5 + k * (1 << PRECISION_BITS)) if k < 0 else int(0.5 + k * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return bounds, kk


def _resample_axis0(img, bounds, kk):
    out = np.empty((bounds.shape[0],) + img.shape[1:], np.uint8)
    x64 = img.astype(np.int64)
    for i in range(bounds.shape[0]):
        xmin, cnt = int(bounds[i, 0]), int(bounds[i, 1])
        acc = np.full(img.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
        for x in range(cnt):
            acc += x64[xmin + x] * int(kk[i, x])
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return out


def resize(img, out_w, out_h, filt):
    """Image.resize((out_w, out_h), filt) of a uint8 [h, w, c] array: horizontal pass, rounded to 8 bits, then vertical; a pass
    whose size does not change is skipped."""
    h, w = img.shape[:2]
    if out_w != w:
        b, k = coeffs(w, out_w, filt)
        img = np.transpose(_resample_axis0(np.transpose(img, (1, 0, 2)), b, k), (1, 0, 2))
    if out_h != h:
        b, k = coeffs(h, out_h, filt)
        img = _resample_axis0(img, b, k)
    return img


def transform_image(img, S, fill, sw, sh, filt=BILINEAR, flip_h=False, flip_v=False, crop=None, ox=0, oy=0):
    """flip -> crop (x0, y0, w, h) -> resize to sw x sh -> window at (ox, oy) -> paste top-left on an S x S canvas: uint8 [3, S, S]."""
    if flip_h:
        img = img[:, ::-1]
    if flip_v:
        img = img[::-1]
    if crop is not None:
        x0, y0, cw, ch = crop
        img = img[y0:y0 + ch, x0:x0 + cw]
    r = resize(np.ascontiguousarray(img), sw, sh, filt)[oy:oy + S, ox:ox + S]
    canvas = np.empty((S, S, 3), np.uint8)
    canvas[:] = np.array(fill, np.uint8)
    canvas[:r.shape[0], :r.shape[1]] = r
    return np.ascontiguousarray(np.transpose(canvas, (2, 0, 1)))


def transform_boxes(boxes, cls, img_w, img_h, scale, flip_h=False, flip_v=False, pre=(0, 0), post=(0, 0), clip=(0, 0)):
    """boxes float32 [M, 4] yxyx, cls int64 [M] (padding rows: class -1, zero box) -> (boxes [M, 4] with the kept rows first and zero
    rows behind, cls [M] with -1 behind, count, valid [M] bool): float32 arithmetic, one rounding per reference operation."""
    b = np.array(boxes, np.float32)
    f = np.float32
    if flip_h:
        x_max, x_min = f(img_w) - b[:, 1], f(img_w) - b[:, 3]
        b[:, 1], b[:, 3] = x_min, x_max
    if flip_v:
        y_max, y_min = f(img_h) - b[:, 0], f(img_h) - b[:, 2]
        b[:, 0], b[:, 2] = y_min, y_max
    b = b - np.array([pre[0], pre[1]] * 2, np.float32)
    b = b * f(scale)
    b = b - np.array([post[0], post[1]] * 2, np.float32)
    b = np.minimum(np.maximum(b, f(0)), np.array([clip[0], clip[1]] * 2, np.float32))
    valid = (b[:, :2] < b[:, 2:4]).all(axis=1)
    n = int(valid.sum())
    ob = np.zeros_like(b)
    oc = np.full(len(b), -1, np.int64)
    ob[:n] = b[valid]
    oc[:n] = np.asarray(cls)[valid]
    return ob, oc, n, valid


# ---- seeded inputs of tests/golden/transforms.npz (tools/make_golden.py::gen_transforms records the reference's outputs for them) ----
TRAIN_SEEDS = tuple(range(12))
TRAIN_S, TRAIN_SCALE = 64, (0.4, 1.7)              # dataloader.py:150 passes (0.4, 1.7)
TRAIN128_SEEDS, TRAIN128_S = (12, 13), 128         # one 2-image batch at the smallest size an EfficientDet-D0 training step takes
EVAL_SEEDS, PROJ_SEEDS, SMALL_S = (0, 1, 2), (0, 1, 2, 3), 32
N_BOXES = 6


def transform_case(kind, seed):
    """-> (image uint8 [h, w, 3] noise, boxes float32 [6, 4] yxyx inside the image, classes int64 [6]); legacy RandomState: the same
    bytes on every numpy."""
    rs = np.random.RandomState({'train': 1000, 'eval': 2000, 'proj': 3000}[kind] + seed)
    lo = 64 if kind == 'proj' else 40
    h, w = int(rs.randint(lo, 81)), int(rs.randint(lo, 81))
    img = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    y0, x0 = rs.uniform(0, 0.85 * h, N_BOXES), rs.uniform(0, 0.85 * w, N_BOXES)
    bh, bw = rs.uniform(2, 0.4 * h, N_BOXES), rs.uniform(2, 0.4 * w, N_BOXES)
    boxes = np.stack([y0, x0, np.minimum(y0 + bh, h), np.minimum(x0 + bw, w)], 1).astype(np.float32)
    cls = rs.randint(1, 5, N_BOXES).astype(np.int64)
    cls[0] = 1                                      # the projection transform draws its object from the boxes of class 1
    return img, boxes, cls
