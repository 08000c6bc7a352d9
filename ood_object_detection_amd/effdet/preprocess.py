"""Device-side input normalisation (reference: `PrefetchLoader`, effdet/data/loader.py:103-146).

The reference's loader hands the model `(uint8 - 255*mean) / (255*std)` computed with torch ops on the GPU
(loader.py:114-128).  Here the same arithmetic is one HIP kernel (`normalize_batch`), or - when a raw uint8
batch is passed straight to `EfficientDet.forward` / `DetBenchPredict.forward` - part of the network's first
kernel (`effdet_stem_dw_fused_u8`), so the normalised tensor is never written to memory.
`EfficientDet.input_mean / input_std` (ImageNet constants by default, `effdet/data/transforms.py:11-12`) are
the constants the fused path uses."""
import collections
import ctypes
import random

import torch

from .. import _lib

IMAGENET_DEFAULT_MEAN = (0.485, 0.456, 0.406)
IMAGENET_DEFAULT_STD = (0.229, 0.224, 0.225)


def normalize_batch(x: torch.Tensor, mean=IMAGENET_DEFAULT_MEAN, std=IMAGENET_DEFAULT_STD, dtype=torch.float32):
    """uint8 [B, C, H, W] on a GPU -> `(x - 255*mean) / (255*std)` as `dtype` (float32 or bfloat16)."""
    if x.dtype != torch.uint8 or x.dim() != 4:
        raise ValueError('expected a uint8 [B, C, H, W] tensor')
    if x.device.type != 'cuda':
        raise RuntimeError('normalize_batch runs on the GPU only (no CPU fallback)')
    if dtype not in (torch.float32, torch.bfloat16):
        raise ValueError('dtype must be float32 or bfloat16')
    B, C, H, W = x.shape
    if len(mean) != C or len(std) != C or C > 4:
        raise ValueError('mean / std must have one entry per channel (at most 4 channels)')
    lib = _lib.load()
    x = x.contiguous()
    y = torch.empty(B, C, H, W, dtype=dtype, device=x.device)
    m = (ctypes.c_float * C)(*[255.0 * v for v in mean])
    s = (ctypes.c_float * C)(*[255.0 * v for v in std])
    st = torch.cuda.current_stream(x.device).cuda_stream
    _lib.check(lib.effdet_normalize_u8(st, 0 if dtype == torch.float32 else 1, x.data_ptr(), m, s, y.data_ptr(), B, C, H * W),
               'effdet_normalize_u8')
    return y


# ---- ResizePad on the device (effdet/data/transforms.py:75-107) --------------------------------------
_PRECISION_BITS = 32 - 8 - 2


def _pil_bilinear_tables(in_size, out_size):
    """Pillow's BILINEAR coefficient tables (Resample.c precompute_coeffs + normalize_coeffs_8bpc), computed in
    float64 with Pillow's operation order: (bounds int32 [out,2], coefficients int32 [out,ksize])."""
    import numpy as np
    if in_size == out_size:                                   # Pillow skips the pass; identity coefficients do the same
        b = np.stack([np.arange(out_size), np.ones(out_size, np.int64)], 1).astype(np.int32)
        return b, np.full((out_size, 1), 1 << _PRECISION_BITS, np.int32)
    scale = float(in_size) / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    xx = np.arange(out_size, dtype=np.float64)
    center = (xx + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)           # C cast: truncation toward zero
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    x = np.arange(ksize, dtype=np.int64)[None, :]
    a = np.abs((x + xmin[:, None] - center[:, None] + 0.5) * ss)
    w = np.where((a < 1.0) & (x < xmax[:, None]), 1.0 - a, 0.0)
    ww = np.zeros(out_size, np.float64)
    for j in range(ksize):                                     # Pillow sums the weights left to right
        ww = ww + w[:, j]
    k = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    kk = np.where(k < 0, (-0.5 + k * (1 << _PRECISION_BITS)).astype(np.int64), (0.5 + k * (1 << _PRECISION_BITS)).astype(np.int64))
    kk = np.where(x < xmax[:, None], kk, 0)
    return np.stack([xmin, xmax], 1).astype(np.int32), kk.astype(np.int32)


def resolve_fill_color(fill_color='mean', img_mean=IMAGENET_DEFAULT_MEAN):
    """effdet/data/transforms.py:279-290."""
    if isinstance(fill_color, tuple):
        assert len(fill_color) == 3
        return fill_color
    try:
        return (int(fill_color),) * 3
    except ValueError:
        assert fill_color == 'mean'
        return tuple(int(round(255 * x)) for x in img_mean)


def resize_pad(img: torch.Tensor, target_size: int, fill_color=(0, 0, 0)):
    """`ResizePad.__call__` for one image: uint8 [h, w, 3] GPU tensor -> (uint8 [3, S, S] ready for the batch,
    img_scale = 1 / scale as stored in anno['img_scale'])."""
    import numpy as np
    if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
        raise ValueError('expected a uint8 [h, w, 3] image')
    if img.device.type != 'cuda':
        raise RuntimeError('resize_pad runs on the GPU only (no CPU fallback)')
    h, w = int(img.shape[0]), int(img.shape[1])
    S = int(target_size)
    img_scale = min(S / h, S / w)
    sh, sw = int(h * img_scale), int(w * img_scale)
    lib = _lib.load()
    dev = img.device
    bx, kx = _pil_bilinear_tables(w, sw)
    by, ky = _pil_bilinear_tables(h, sh)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    bxd, kxd, byd, kyd = t(bx), t(kx), t(by), t(ky)
    img = img.contiguous()
    out = torch.empty(3, S, S, dtype=torch.uint8, device=dev)
    ws = torch.empty(h * sw * 3, dtype=torch.uint8, device=dev)
    fill = (ctypes.c_int * 3)(*[int(v) for v in fill_color])
    st = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(lib.effdet_resize_pad_u8(st, img.data_ptr(), h, w, out.data_ptr(), S, sw, sh, bxd.data_ptr(), kxd.data_ptr(), kx.shape[1],
                                        byd.data_ptr(), kyd.data_ptr(), ky.shape[1], fill, ws.data_ptr()), 'effdet_resize_pad_u8')
    return out, 1.0 / img_scale


# ---- the transforms of effdet/data/transforms.py for a whole batch on the device ---------------------------------------
# One launch of effdet_resample_batch_u8 makes the [B, 3, S, S] uint8 network input from a ragged list of frames, one launch of
# effdet_transform_boxes does the box arithmetic; the host only draws the random parameters (double arithmetic, as the
# reference) and uploads them in ONE pinned buffer.  Nothing is read back and nothing synchronises.
BILINEAR, BICUBIC = 0, 1
_FILTERS = {'bilinear': BILINEAR, 'bicubic': BICUBIC}


class TransformParams(collections.namedtuple('TransformParams', [
        'sw', 'sh', 'scale', 'flip_h', 'flip_v', 'crop', 'filter', 'ox', 'oy', 'pre_offset', 'post_offset', 'clip'])):
    """One image's transform.  Pixels: mirror (`flip_h`, `flip_v`), crop `(x0, y0, w, h)` of the mirrored frame (None: all of it),
    resample to `sw` x `sh` with `filter` (BILINEAR / BICUBIC), window at (`ox`, `oy`), paste top-left.  Boxes (yxyx, float32):
    mirror, subtract `pre_offset` (y, x), multiply by float32(`scale`), subtract `post_offset` (y, x), clip to `clip` (h, w).
    `scale` is the reference's img_scale (a Python float); anno['img_scale'] = 1 / scale."""
    __slots__ = ()

    def __new__(cls, sw, sh, scale, flip_h=False, flip_v=False, crop=None, filter=BILINEAR, ox=0, oy=0, pre_offset=(0, 0),
                post_offset=(0, 0), clip=None):
        return super().__new__(cls, int(sw), int(sh), float(scale), bool(flip_h), bool(flip_v), crop, int(filter), int(ox), int(oy),
                               pre_offset, post_offset, (sh, sw) if clip is None else clip)


Transformed = collections.namedtuple('Transformed', ['batch', 'img_info', 'boxes', 'cls', 'counts', 'valid_indices'])

_DESC = [('src', '<u8'), ('h', '<i4'), ('w', '<i4'), ('flip_h', '<i4'), ('flip_v', '<i4'), ('cx0', '<i4'), ('cy0', '<i4'),
         ('cw', '<i4'), ('ch', '<i4'), ('filter', '<i4'), ('sw', '<i4'), ('sh', '<i4'), ('ox', '<i4'), ('oy', '<i4'), ('reserved', '<i4')]
_BOXP = [('img_w', '<f4'), ('img_h', '<f4'), ('flip_h', '<i4'), ('flip_v', '<i4'), ('pre_y', '<f4'), ('pre_x', '<f4'), ('scale', '<f4'),
         ('post_y', '<f4'), ('post_x', '<f4'), ('clip_h', '<f4'), ('clip_w', '<f4'), ('reserved', '<i4')]


def _pack_params(images, params):
    """-> (images kept alive, pinned host buffer, its device copy, byte sizes of the descriptor and box-parameter parts): the
    call's ONE upload - B descriptors, B box parameter records, img_scale [B], img_size [B, 2]."""
    import numpy as np
    B = len(images)
    if B == 0 or len(params) != B:
        raise ValueError('one TransformParams per image')
    dev = images[0].device
    if dev.type != 'cuda':
        raise RuntimeError('apply_transforms runs on the GPU only (no CPU fallback)')
    keep = []
    for im in images:
        if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3 or im.device != dev:
            raise ValueError('expected uint8 [h, w, 3] images on one GPU')
        keep.append(im if im.stride() == (3 * im.shape[1], 3, 1) else im.contiguous())
    nd, nb = 64 * B, 48 * B
    host = torch.empty(nd + nb + 12 * B, dtype=torch.uint8, pin_memory=True)
    raw = host.numpy()
    desc, boxp = raw[:nd].view(_DESC), raw[nd:nd + nb].view(_BOXP)
    inv, size = raw[nd + nb:nd + nb + 4 * B].view('<f4'), raw[nd + nb + 4 * B:].view('<f4').reshape(B, 2)
    raw[:nd + nb] = 0
    for i, (im, p) in enumerate(zip(keep, params)):
        h, w = int(im.shape[0]), int(im.shape[1])
        cx0, cy0, cw, ch = (0, 0, w, h) if p.crop is None else [int(v) for v in p.crop]
        desc[i] = (im.data_ptr(), h, w, p.flip_h, p.flip_v, cx0, cy0, cw, ch, p.filter, p.sw, p.sh, p.ox, p.oy, 0)
        boxp[i] = (w, h, p.flip_h, p.flip_v, p.pre_offset[0], p.pre_offset[1], p.scale, p.post_offset[0], p.post_offset[1],
                   p.clip[0], p.clip[1], 0)
        inv[i] = 1.0 / p.scale
        size[i] = (w, h)
    return keep, host, host.to(dev, non_blocking=True), nd, nb


def apply_transforms(images, params, target_size, fill_color=(0, 0, 0), boxes=None, classes=None, out=None):
    """images: list of uint8 [h, w, 3] GPU tensors (rows packed; any byte offset, e.g. views into one buffer); params: one
    `TransformParams` per image -> `Transformed`: `batch` uint8 [B, 3, S, S] (written into `out` when given: a [B, 3, S, S] uint8
    tensor or slice whose images are contiguous), `img_info` = {'img_scale': float32 [B], 'img_size': float32 [B, 2] (width,
    height)} as `DetBenchPredict(x, img_info=...)` takes it, and - when `boxes` float32 [B, Mmax, 4] yxyx / `classes` int64
    [B, Mmax] (padding rows: class -1, zero box) are given - the kept rows compacted in order (`boxes`, `cls`), `counts` int32 [B]
    and `valid_indices` bool [B, Mmax] aligned with the input rows."""
    B, S = len(images), int(target_size)
    if (boxes is None) != (classes is None):
        raise ValueError('boxes and classes go together')
    keep, host, devbuf, nd, nb = _pack_params(images, params)
    dev = devbuf.device
    lib = _lib.load()
    if out is None:
        out = torch.empty(B, 3, S, S, dtype=torch.uint8, device=dev)
    elif (out.dtype != torch.uint8 or tuple(out.shape) != (B, 3, S, S) or out.device != dev or not out[0].is_contiguous()
          or (B > 1 and out.stride(0) < 3 * S * S)):
        raise ValueError('out must be a uint8 [B, 3, S, S] tensor on the images\' GPU with contiguous images')
    fill = (ctypes.c_int * 3)(*[int(v) for v in fill_color])
    st = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(lib.effdet_resample_batch_u8(st, devbuf.data_ptr(), host.data_ptr(), B, out.data_ptr(),
                                            out.stride(0) if B > 1 else 3 * S * S, S, fill), 'effdet_resample_batch_u8')
    info = {'img_scale': devbuf[nd + nb:nd + nb + 4 * B].view(torch.float32),
            'img_size': devbuf[nd + nb + 4 * B:].view(torch.float32).reshape(B, 2)}
    if boxes is None:
        return Transformed(out, info, None, None, None, None)
    if (boxes.dtype != torch.float32 or boxes.dim() != 3 or boxes.shape[0] != B or boxes.shape[2] != 4 or classes.dtype != torch.int64
            or tuple(classes.shape) != tuple(boxes.shape[:2]) or boxes.device != dev or classes.device != dev):
        raise ValueError('boxes float32 [B, Mmax, 4] and classes int64 [B, Mmax] on the images\' GPU')
    M = int(boxes.shape[1])
    boxes, classes = boxes.contiguous(), classes.contiguous()
    ob, oc = torch.empty_like(boxes), torch.empty_like(classes)
    cnt = torch.empty(B, dtype=torch.int32, device=dev)
    valid = torch.empty(B, M, dtype=torch.bool, device=dev)
    _lib.check(lib.effdet_transform_boxes(st, boxes.data_ptr(), classes.data_ptr(), devbuf.data_ptr() + nd, B, M, ob.data_ptr(),
                                          oc.data_ptr(), cnt.data_ptr(), valid.data_ptr()), 'effdet_transform_boxes')
    return Transformed(out, info, ob, oc, cnt, valid)


def _filter_id(interpolation):
    if interpolation not in _FILTERS:                          # the reference also knows lanczos / hamming (transforms.py:40-49): not built
        raise ValueError('interpolation must be \'bilinear\' or \'bicubic\' (or \'random\' where the transform draws it)')
    return _FILTERS[interpolation]


def resize_pad_params(sizes, target_size, interpolation='bilinear'):
    """`ResizePad` (transforms.py:82-105) for images of `sizes` [(h, w), ...]."""
    S, out = int(target_size), []
    for h, w in sizes:
        s = min(S / h, S / w)
        out.append(TransformParams(int(w * s), int(h * s), s, filter=_filter_id(interpolation)))
    return out


def resize_pad_batch(images, target_size, fill_color=(0, 0, 0), boxes=None, classes=None, interpolation='bilinear', out=None):
    """`transforms_coco_eval` for a batch: see `apply_transforms`."""
    prm = resize_pad_params([(int(im.shape[0]), int(im.shape[1])) for im in images], target_size, interpolation)
    return apply_transforms(images, prm, target_size, fill_color, boxes, classes, out)


def draw_train_params(sizes, target_size, scale, interpolation='random', horizontal=True, rng=random):
    """The host-side draws of `transforms_coco_train` for images of `sizes` [(h, w), ...]: `RandomFlip._get_params`
    (transforms.py:241-244), `RandomResizePad._get_params` (:182-201) and the filter choice (:206-209), per image in the
    reference's order - rng.random(), rng.uniform(*scale), rng.uniform(0, 1) for y then x, rng.choice - and in its double
    arithmetic, so a seeded `random` gives the reference's parameters."""
    S, out = int(target_size), []
    for h, w in sizes:
        flip = rng.random() < 0.5 if horizontal else False
        scale_factor = rng.uniform(*scale)
        img_scale = min(scale_factor * S / h, scale_factor * S / w)
        sh, sw = int(h * img_scale), int(w * img_scale)
        oy = int(max(0.0, float(sh - S)) * rng.uniform(0, 1))
        ox = int(max(0.0, float(sw - S)) * rng.uniform(0, 1))
        filt = rng.choice((BILINEAR, BICUBIC)) if interpolation == 'random' else _filter_id(interpolation)
        out.append(TransformParams(sw, sh, img_scale, flip_h=flip, filter=filt, ox=ox, oy=oy, post_offset=(oy, ox)))
    return out


def random_resize_pad_batch(images, target_size, scale, fill_color=(0, 0, 0), boxes=None, classes=None, interpolation='random',
                            horizontal=True, rng=random, out=None):
    """`transforms_coco_train` for a batch (`scale`: the range the data set passes per call, transforms.py:184)."""
    prm = draw_train_params([(int(im.shape[0]), int(im.shape[1])) for im in images], target_size, scale, interpolation, horizontal, rng)
    return apply_transforms(images, prm, target_size, fill_color, boxes, classes, out)


def proj_params(crops, flips, target_size, interpolation='bilinear'):
    """`ProjResizePad`'s arithmetic (transforms.py:143-160) for GIVEN crop boxes (x0, y0, x1, y1) of the (mirrored) image."""
    S, out = int(target_size), []
    for (x0, y0, x1, y1), flip in zip(crops, flips):
        cw, ch = int(x1) - int(x0), int(y1) - int(y0)
        s = min(S / cw, S / ch)
        out.append(TransformParams(int(s * cw), int(s * ch), s, flip_h=flip, crop=(int(x0), int(y0), cw, ch),
                                   filter=_filter_id(interpolation), pre_offset=(int(y0), int(x0))))
    return out


def proj_resize_pad_batch(images, crops, flips, target_size, fill_color=(0, 0, 0), boxes=None, classes=None,
                          interpolation='bilinear', out=None):
    """`transforms_projection` for a batch with the crop rectangles supplied by the caller (the reference draws them from the
    box list, transforms.py:127-141); `flips`: RandomFlip's horizontal decision per image, applied before the crop."""
    return apply_transforms(images, proj_params(crops, flips, target_size, interpolation), target_size, fill_color, boxes, classes, out)
