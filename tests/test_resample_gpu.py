"""The batched transforms on the device (effdet/preprocess.py::apply_transforms and its three entry points, csrc/resample.hip)
against tests/_pil_ref.py - pinned to PIL and to the reference's pipelines by tests/test_resample_host.py - and against the
reference's recorded outputs in tests/golden/transforms.npz.  Everything here is integer- or float32-exact: no tolerances."""
import copy
import functools
import random

import numpy as np
import pytest
import torch

import _pil_ref as R

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
FILL = (124, 116, 104)                                      # resolve_fill_color('mean')


def _P():
    from ood_object_detection_amd.effdet import preprocess as P
    return P


def _noise(seed, h, w):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def _ref_image(img, p, S):
    return R.transform_image(img, S, FILL, p.sw, p.sh, p.filter, p.flip_h, p.flip_v, p.crop, p.ox, p.oy)


def _check_images(imgs, params, S, dev_imgs=None, out=None):
    P = _P()
    dev_imgs = [torch.from_numpy(im).to(DEV) for im in imgs] if dev_imgs is None else dev_imgs
    t = P.apply_transforms(dev_imgs, params, S, FILL, out=out)
    got = t.batch.cpu().numpy()
    for i, (im, p) in enumerate(zip(imgs, params)):
        assert np.array_equal(got[i], _ref_image(im, p, S)), (i, im.shape, p)
    return t


RAGGED = [(37, 53), (200, 150), (61, 61), (300, 17), (13, 9), (1, 7), (5, 1)]


# ---- 1. one ragged call --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('S', [64, 40])
def test_ragged_batch_both_filters(S):
    """upscale, downscale, an identity pass, a 17 : 1 reduction with a 3-pixel pasted width, one-pixel sources - every image with
    both filters in ONE call; S = 40 is not a tile multiple, so the extents end inside a tile"""
    P = _P()
    imgs = [_noise(10 + i, h, w) for i, (h, w) in enumerate(RAGGED)] * 2
    params = P.resize_pad_params(RAGGED, S, 'bilinear') + P.resize_pad_params(RAGGED, S, 'bicubic')
    assert {p.filter for p in params} == {0, 1}
    t = _check_images(imgs, params, S)
    assert t.img_info['img_scale'].dtype == torch.float32 and tuple(t.img_info['img_size'].shape) == (len(imgs), 2)
    assert t.img_info['img_scale'].cpu().tolist() == [float(np.float32(1.0 / p.scale)) for p in params]
    assert t.img_info['img_size'].cpu().tolist() == [[float(w), float(h)] for h, w in RAGGED * 2]


def test_result_does_not_depend_on_the_batch():
    P = _P()
    imgs = [_noise(20 + i, h, w) for i, (h, w) in enumerate(RAGGED)]
    params = P.resize_pad_params(RAGGED, 64, 'bicubic')
    dev = [torch.from_numpy(im).to(DEV) for im in imgs]
    whole = P.apply_transforms(dev, params, 64, FILL).batch
    for i in (0, 3, 6):
        assert torch.equal(P.apply_transforms([dev[i]], [params[i]], 64, FILL).batch[0], whole[i])


def test_large_reductions_and_the_documented_limit():
    """64 : 1 on both axes with the 257-tap bicubic filter (the LDS plan's smallest tile), 40 : 1 bilinear; beyond 64 : 1 is refused"""
    P = _P()
    img = _noise(3, 640, 704)
    _check_images([img, img], [P.TransformParams(11, 10, 1.0, filter=P.BICUBIC), P.TransformParams(70, 16, 1.0, filter=P.BILINEAR)], 64)
    with pytest.raises(RuntimeError):
        P.apply_transforms([torch.from_numpy(img).to(DEV)], [P.TransformParams(10, 10, 1.0)], 64, FILL)


# ---- 2. train-style windows ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('flip', [False, True])
def test_train_windows(flip):
    """scaled image larger than the canvas with a window offset on both axes; extents cut by S on one axis only; vertical flip"""
    P = _P()
    imgs = [_noise(30, 90, 100), _noise(31, 100, 60), _noise(32, 60, 130), _noise(33, 50, 70)]
    params = [P.TransformParams(138, 124, 1.0, flip_h=flip, filter=P.BICUBIC, ox=37, oy=21),
              P.TransformParams(50, 141, 1.0, flip_h=flip, filter=P.BILINEAR, ox=0, oy=70),       # cut by S vertically only
              P.TransformParams(150, 53, 1.0, flip_h=flip, filter=P.BICUBIC, ox=86, oy=0),        # cut by S horizontally only
              P.TransformParams(99, 80, 1.0, flip_h=flip, flip_v=True, filter=P.BILINEAR, ox=60, oy=30)]   # window ends inside the canvas
    _check_images(imgs, params, 64)


def _fixture_batch(g, kind, seeds, S, params_of):
    """device call on the seeded inputs of the fixture cases -> (Transformed, inputs)"""
    P = _P()
    cases = [R.transform_case(kind, s) for s in seeds]
    params = [params_of(s, c[0]) for s, c in zip(seeds, cases)]
    M = R.N_BOXES + 2                                        # two padding rows behind every image's boxes
    boxes = torch.zeros(len(seeds), M, 4)
    cls = torch.full((len(seeds), M), -1, dtype=torch.int64)
    for i, (_, b, c) in enumerate(cases):
        boxes[i, :R.N_BOXES], cls[i, :R.N_BOXES] = torch.from_numpy(b), torch.from_numpy(c)
    t = P.apply_transforms([torch.from_numpy(c[0]).to(DEV) for c in cases], params, S, FILL, boxes.to(DEV), cls.to(DEV))
    return t, params


def _check_fixture(g, tag, seeds, t, with_valid=True):
    for i, s in enumerate(seeds):
        key = '%s%d_' % (tag, s)
        assert np.array_equal(t.batch[i].cpu().numpy(), g[key + 'img']), key
        n = int(t.counts[i])
        assert n == len(g[key + 'obox'])
        assert np.array_equal(t.boxes[i, :n].cpu().numpy(), g[key + 'obox']) and np.array_equal(t.cls[i, :n].cpu().numpy(), g[key + 'ocls'])
        assert not t.boxes[i, n:].any() and bool((t.cls[i, n:] == -1).all())
        if with_valid:
            assert np.array_equal(t.valid_indices[i, :R.N_BOXES].cpu().numpy(), g[key + 'valid']) and not t.valid_indices[i, R.N_BOXES:].any()
        assert float(t.img_info['img_scale'][i]) == float(np.float32(g[key + 'img_scale']))


def _train_draw(seed, img, S):
    random.seed(seed)
    return _P().draw_train_params([img.shape[:2]], S, R.TRAIN_SCALE, rng=random)[0]


def test_train_fixture(golden):
    """transforms_coco_train end to end: images, boxes, classes, valid_indices and img_scale equal the reference's recorded outputs"""
    g = golden('transforms')
    t, params = _fixture_batch(g, 'train', R.TRAIN_SEEDS, R.TRAIN_S, lambda s, im: _train_draw(s, im, R.TRAIN_S))
    assert {p.filter for p in params} == {0, 1} and {p.flip_h for p in params} == {False, True}
    _check_fixture(g, 'train', R.TRAIN_SEEDS, t)


def test_eval_fixture(golden):
    g = golden('transforms')
    P = _P()
    t, _ = _fixture_batch(g, 'eval', R.EVAL_SEEDS, R.SMALL_S, lambda s, im: P.resize_pad_params([im.shape[:2]], R.SMALL_S)[0])
    _check_fixture(g, 'eval', R.EVAL_SEEDS, t, with_valid=False)


# ---- 3. projection -------------------------------------------------------------------------------------------------------------

def test_projection_fixture(golden):
    g = golden('transforms')
    P = _P()

    def params_of(s, im):
        flip, filt, sw, sh, x0, y0, x1, y1 = [int(v) for v in g['proj%d_params' % s]]
        return P.proj_params([(x0, y0, x1, y1)], [flip], R.SMALL_S)[0]
    t, _ = _fixture_batch(g, 'proj', R.PROJ_SEEDS, R.SMALL_S, params_of)
    _check_fixture(g, 'proj', R.PROJ_SEEDS, t)


@pytest.mark.parametrize('filt', [0, 1])
def test_crop_bounds_clamp_to_the_crop(filt):
    """a crop strictly inside the image: its edge rows and columns must not see the pixels beyond it.  The same call on an image
    whose pixels OUTSIDE the crop are different gives the same bytes, and both equal the yardstick."""
    P = _P()
    img = _noise(40, 70, 90)
    crops, flips = [(11, 7, 71, 57), (20, 10, 85, 70)], [True, False]
    params = P.proj_params(crops, flips, 48, ('bilinear', 'bicubic')[filt])
    t = _check_images([img, img], params, 48)
    others = []
    for (x0, y0, x1, y1), flip in zip(crops, flips):
        o = _noise(41, 70, 90)
        view, src = (o[:, ::-1], img[:, ::-1]) if flip else (o, img)
        view[y0:y1, x0:x1] = src[y0:y1, x0:x1]
        others.append(o)
    assert torch.equal(P.apply_transforms([torch.from_numpy(o).to(DEV) for o in others], params, 48, FILL).batch, t.batch)


# ---- 4. alignment --------------------------------------------------------------------------------------------------------------

def test_sources_at_any_byte_offset_and_output_slice():
    """the same images as views into one byte buffer at offsets 1, 2 and 3 mod 4 (and widths with 3 * w odd, so that the row
    alignment changes from row to row), written into a slice of a larger batch tensor"""
    P = _P()
    shapes = [(37, 53), (61, 61), (200, 151), (13, 9)]
    imgs = [_noise(50 + i, h, w) for i, (h, w) in enumerate(shapes)]
    params = P.resize_pad_params(shapes, 64, 'bicubic')
    aligned = P.apply_transforms([torch.from_numpy(im).to(DEV) for im in imgs], params, 64, FILL).batch
    for first in (1, 2, 3):
        buf, views, pos = torch.empty(sum(im.size for im in imgs) + 64, dtype=torch.uint8, device=DEV), [], first
        for im in imgs:
            v = buf[pos:pos + im.size].view(im.shape)
            v.copy_(torch.from_numpy(im))
            views.append(v)
            pos += im.size + (1 if im.size % 2 == 0 else 2)                 # the next image starts at another offset mod 4
        assert {v.data_ptr() % 4 for v in views} != {0}
        big = torch.full((len(imgs) + 3, 3, 64, 64), 7, dtype=torch.uint8, device=DEV)
        t = _check_images(imgs, params, 64, dev_imgs=views, out=big[2:2 + len(imgs)])
        assert t.batch.data_ptr() == big[2].data_ptr() and torch.equal(big[2:2 + len(imgs)], aligned)
        assert bool((big[:2] == 7).all()) and bool((big[2 + len(imgs):] == 7).all())


def test_canvas_size_that_is_no_multiple_of_four():
    """S = 37: plane rows are not 4-byte aligned, the stores fall back to bytes"""
    P = _P()
    shapes = [(37, 53), (200, 150), (20, 37)]
    _check_images([_noise(60 + i, h, w) for i, (h, w) in enumerate(shapes)], P.resize_pad_params(shapes, 37, 'bicubic'), 37)


# ---- 5. boxes alone ------------------------------------------------------------------------------------------------------------

def _run_boxes(boxes, cls, params, sizes):
    """through apply_transforms on blank frames of the given (h, w): the box kernel reads only the parameters"""
    P = _P()
    imgs = [torch.zeros(h, w, 3, dtype=torch.uint8, device=DEV) for h, w in sizes]
    t = P.apply_transforms(imgs, params, 8, FILL, torch.from_numpy(boxes).to(DEV), torch.from_numpy(cls).to(DEV))
    for i, (p, (h, w)) in enumerate(zip(params, sizes)):
        rb, rc, n, valid = R.transform_boxes(boxes[i], cls[i], w, h, p.scale, p.flip_h, p.flip_v, p.pre_offset, p.post_offset, p.clip)
        assert int(t.counts[i]) == n
        assert np.array_equal(t.boxes[i].cpu().numpy(), rb) and np.array_equal(t.cls[i].cpu().numpy(), rc)
        assert np.array_equal(t.valid_indices[i].cpu().numpy(), valid)
    return t


def test_boxes_edges():
    """boxes exactly on the clip edge, zero area after clipping, all boxes dropped, padding rows left alone, order preserved"""
    P = _P()
    sizes = [(40, 60), (40, 60), (40, 60)]
    p0 = P.TransformParams(30, 20, 0.5, flip_h=True, post_offset=(2, 3), clip=(20, 30))
    p1 = P.TransformParams(30, 20, 0.5, flip_v=True, pre_offset=(4, 6), clip=(18, 27))
    p2 = P.TransformParams(8, 8, 0.25, post_offset=(30, 30), clip=(8, 8))                       # everything lands left of / above the window
    M = 9
    boxes = np.zeros((3, M, 4), np.float32)
    cls = np.full((3, M), -1, np.int64)
    boxes[0, :7] = [[4, 6, 44, 66],        # flipped and scaled to exactly the clip rectangle's far edge and beyond
                    [4, 0, 4.5, 60],       # thin but not empty
                    [0, 0, 4, 6],          # scales to (0,27)..(2,30): minus the offset it clips to zero height -> dropped
                    [10, 54, 30, 54],      # zero width
                    [39, 1, 40, 2],
                    [44, 66, 50, 70],      # wholly beyond the clip edge -> zero area at the edge
                    [6, 8, 30, 40]]
    cls[0, :7] = [5, 4, 3, 2, 1, 9, 8]
    boxes[1, :6] = [[4, 6, 40, 60], [0, 0, 40, 60], [36, 6, 40, 10], [3.5, 5.5, 4, 6], [20, 20, 20.001, 59], [10, 10, 30, 30]]
    cls[1, :6] = [1, 2, 3, 4, 5, 6]
    boxes[2, :5] = [[1, 1, 20, 20], [5, 5, 100, 100], [0, 0, 40, 60], [30, 30, 31, 31], [2, 50, 12, 58]]
    cls[2, :5] = [7, 7, 7, 7, 7]
    t = _run_boxes(boxes, cls, [p0, p1, p2], sizes)
    assert 0 < int(t.counts[0]) < 7 and 0 < int(t.counts[1]) < 6 and int(t.counts[2]) == 0
    assert not t.boxes[2].any() and bool((t.cls[2] == -1).all())
    kept = t.cls[0, :int(t.counts[0])].cpu().tolist()
    assert kept == [c for c in [5, 4, 3, 2, 1, 9, 8] if c in kept]                             # original order


@pytest.mark.parametrize('M', [1, 512])
def test_boxes_mmax(M):
    P = _P()
    rs = np.random.RandomState(M)
    B = 3
    y0, x0 = rs.uniform(0, 90, (B, M)), rs.uniform(0, 120, (B, M))
    boxes = np.stack([y0, x0, y0 + rs.uniform(0, 40, (B, M)), x0 + rs.uniform(0, 40, (B, M))], -1).astype(np.float32)
    cls = rs.randint(1, 90, (B, M)).astype(np.int64)
    if M > 1:
        boxes[1, M // 2:], cls[1, M // 2:] = 0, -1                                            # an image with padding rows
    params = [P.TransformParams(100, 80, 0.83, flip_h=True, ox=17, oy=9, post_offset=(9, 17)),
              P.TransformParams(64, 48, 0.53, clip=(48, 64)),
              P.TransformParams(150, 110, 1.25, flip_h=True, flip_v=True, pre_offset=(12, 20), post_offset=(40, 30), clip=(110, 150))]
    t = _run_boxes(boxes, cls, params, [(100, 120)] * B)
    if M > 1:
        assert 0 < int(t.counts[0]) < M


# ---- 6. consumers --------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _d0_128():
    from _models import seeded_model
    return seeded_model('tf_efficientdet_d0', 128, 20, seed=11)[0]


def test_pretrain_step_on_the_device_transformed_batch(golden):
    """PretrainStep (d0, 128 px, 2 images, labels assigned on the device) fed the device-transformed batch - padded boxes and
    classes straight from the box kernel, nothing read back - gives bit for bit the loss it gives on the reference's arrays"""
    from ood_object_detection_amd.pretrain import PretrainStep
    g = golden('transforms')
    seeds, S = R.TRAIN128_SEEDS, R.TRAIN128_S
    t, _ = _fixture_batch(g, 'train', seeds, S, lambda s, im: _train_draw(s, im, S))
    _check_fixture(g, 'train', seeds, t)
    losses = []
    for fed in ('device', 'fixture'):
        step = PretrainStep(copy.deepcopy(_d0_128()).to(DEV).float())
        if fed == 'device':
            x, target = t.batch, {'bbox': list(t.boxes), 'cls': list(t.cls)}
        else:
            x = torch.from_numpy(np.stack([g['train%d_img' % s] for s in seeds])).to(DEV)
            target = {'bbox': [torch.from_numpy(g['train%d_obox' % s]).to(DEV) for s in seeds],
                      'cls': [torch.from_numpy(g['train%d_ocls' % s]).to(DEV) for s in seeds]}
        out = step(x, target)
        losses.append([out[k].item() for k in ('loss', 'class_loss', 'box_loss')])
    assert np.isfinite(losses[0]).all() and losses[0][2] > 0
    assert losses[0] == losses[1]


def test_det_bench_predict_takes_the_returned_img_info():
    from ood_object_detection_amd.effdet.bench import DetBenchPredict
    P = _P()
    shapes = [(97, 131), (200, 150)]
    imgs = [torch.from_numpy(_noise(70 + i, h, w)).to(DEV) for i, (h, w) in enumerate(shapes)]
    t = P.resize_pad_batch(imgs, 128, FILL)
    bench = DetBenchPredict(copy.deepcopy(_d0_128()).to(DEV).float()).to(DEV)
    got = bench(t.batch, img_info=t.img_info).clone()
    by_hand = {'img_scale': torch.tensor([1.0 / min(128 / h, 128 / w) for h, w in shapes]),
               'img_size': torch.tensor([[float(w), float(h)] for h, w in shapes])}
    ref = bench(t.batch, img_info={k: v.to(DEV) for k, v in by_hand.items()})
    assert torch.equal(got, ref) and bool(got[..., 4].max() > 0)


# ---- 7. the one-image path -----------------------------------------------------------------------------------------------------

def test_equals_resize_pad():
    """the shapes of tests/test_kernels_gpu.py::test_resize_pad_u8 in one batched call against the per-image `resize_pad`"""
    P = _P()
    shapes = [(480, 640), (333, 500), (64, 48), (100, 37), (128, 128), (720, 1280)]
    imgs = [torch.from_numpy(_noise(h * 7 + w, h, w)).to(DEV) for h, w in shapes]
    t = P.resize_pad_batch(imgs, 128, FILL)
    for i, im in enumerate(imgs):
        one, inv = P.resize_pad(im, 128, FILL)
        assert torch.equal(t.batch[i], one)
        assert float(t.img_info['img_scale'][i]) == float(np.float32(inv))
