"""The yardstick of the batched transforms (tests/_pil_ref.py) against PIL itself and against what the reference's own transform
pipelines produced (tests/golden/transforms.npz), and the host-side parameter draws of the product against the same fixture.
No GPU."""
import random

import numpy as np
import pytest

import _pil_ref as R

FILL = (124, 116, 104)                                     # resolve_fill_color('mean')


@pytest.mark.parametrize('filt', [R.BILINEAR, R.BICUBIC])
@pytest.mark.parametrize('shape', [(37, 53, 90, 120), (200, 150, 64, 48), (61, 61, 61, 30), (300, 17, 40, 17), (97, 131, 13, 9)])
def test_resample_matches_pil(shape, filt):
    """(h, w -> oh, ow): up, down, a skipped pass per axis, a 17 : 1 reduction"""
    Image = pytest.importorskip('PIL.Image')
    h, w, oh, ow = shape
    img = np.random.RandomState(h * 1000 + w).randint(0, 256, (h, w, 3)).astype(np.uint8)
    ref = np.asarray(Image.fromarray(img).resize((ow, oh), (Image.BILINEAR, Image.BICUBIC)[filt]))
    assert np.array_equal(R.resize(img, ow, oh, filt), ref)


@pytest.mark.parametrize('filt', [R.BILINEAR, R.BICUBIC])
def test_crop_then_resize_matches_pil(filt):
    """bounds clamp to the crop: the rows and columns next to its edge must not see the pixels outside it"""
    Image = pytest.importorskip('PIL.Image')
    img = np.random.RandomState(7).randint(0, 256, (70, 90, 3)).astype(np.uint8)
    x0, y0, cw, ch = 11, 7, 60, 50
    pim = Image.fromarray(img).transpose(Image.FLIP_LEFT_RIGHT).crop((x0, y0, x0 + cw, y0 + ch))
    canvas = Image.new('RGB', (48, 48), color=FILL)
    canvas.paste(pim.resize((40, 33), (Image.BILINEAR, Image.BICUBIC)[filt]))
    got = R.transform_image(img, 48, FILL, 40, 33, filt, flip_h=True, crop=(x0, y0, cw, ch))
    assert np.array_equal(got, np.transpose(np.asarray(canvas), (2, 0, 1)))
    other = np.random.RandomState(8).randint(0, 256, img.shape).astype(np.uint8)            # new pixels everywhere but in the crop
    other[:, ::-1][y0:y0 + ch, x0:x0 + cw] = img[:, ::-1][y0:y0 + ch, x0:x0 + cw]
    assert np.array_equal(R.transform_image(other, 48, FILL, 40, 33, filt, flip_h=True, crop=(x0, y0, cw, ch)), got)


def _train_params(P, seed, S):
    img, boxes, cls = R.transform_case('train', seed)
    random.seed(seed)
    return img, boxes, cls, P.draw_train_params([img.shape[:2]], S, R.TRAIN_SCALE, rng=random)[0]


@pytest.mark.parametrize('seed', R.TRAIN_SEEDS + R.TRAIN128_SEEDS)
def test_train_draws_and_yardstick_match_reference(golden, seed):
    """`draw_train_params` under a seeded `random` gives the parameters the reference called PIL with, and the yardstick applied
    to them gives the reference's image, boxes, classes, valid_indices and img_scale"""
    from ood_object_detection_amd.effdet import preprocess as P
    g = golden('transforms')
    S = R.TRAIN128_S if seed in R.TRAIN128_SEEDS else R.TRAIN_S
    img, boxes, cls, p = _train_params(P, seed, S)
    flip, filt, sw, sh, ox, oy = [int(v) for v in g['train%d_params' % seed]]
    assert (int(p.flip_h), p.filter, p.sw, p.sh, p.ox, p.oy) == (flip, filt, sw, sh, ox, oy)
    assert 1.0 / p.scale == float(g['train%d_img_scale' % seed])
    assert np.array_equal(R.transform_image(img, S, FILL, p.sw, p.sh, p.filter, p.flip_h, ox=p.ox, oy=p.oy), g['train%d_img' % seed])
    ob, oc, n, valid = R.transform_boxes(boxes, cls, img.shape[1], img.shape[0], p.scale, p.flip_h, post=p.post_offset, clip=p.clip)
    assert np.array_equal(valid, g['train%d_valid' % seed])
    assert np.array_equal(ob[:n], g['train%d_obox' % seed]) and np.array_equal(oc[:n], g['train%d_ocls' % seed])


@pytest.mark.parametrize('seed', R.EVAL_SEEDS)
def test_eval_yardstick_matches_reference(golden, seed):
    from ood_object_detection_amd.effdet import preprocess as P
    g = golden('transforms')
    img, boxes, cls = R.transform_case('eval', seed)
    p = P.resize_pad_params([img.shape[:2]], R.SMALL_S)[0]
    assert 1.0 / p.scale == float(g['eval%d_img_scale' % seed])
    assert np.array_equal(R.transform_image(img, R.SMALL_S, FILL, p.sw, p.sh), g['eval%d_img' % seed])
    ob, oc, n, _ = R.transform_boxes(boxes, cls, img.shape[1], img.shape[0], p.scale, clip=p.clip)
    assert np.array_equal(ob[:n], g['eval%d_obox' % seed]) and np.array_equal(oc[:n], g['eval%d_ocls' % seed])


@pytest.mark.parametrize('seed', R.PROJ_SEEDS)
def test_projection_yardstick_matches_reference(golden, seed):
    from ood_object_detection_amd.effdet import preprocess as P
    g = golden('transforms')
    img, boxes, cls = R.transform_case('proj', seed)
    flip, filt, sw, sh, x0, y0, x1, y1 = [int(v) for v in g['proj%d_params' % seed]]
    p = P.proj_params([(x0, y0, x1, y1)], [flip], R.SMALL_S)[0]
    assert (p.sw, p.sh, p.filter) == (sw, sh, filt) and 1.0 / p.scale == float(g['proj%d_img_scale' % seed])
    assert np.array_equal(R.transform_image(img, R.SMALL_S, FILL, p.sw, p.sh, p.filter, p.flip_h, crop=p.crop), g['proj%d_img' % seed])
    ob, oc, n, valid = R.transform_boxes(boxes, cls, img.shape[1], img.shape[0], p.scale, p.flip_h, pre=p.pre_offset, clip=p.clip)
    assert np.array_equal(valid, g['proj%d_valid' % seed])
    assert np.array_equal(ob[:n], g['proj%d_obox' % seed]) and np.array_equal(oc[:n], g['proj%d_ocls' % seed])


def test_fixture_covers_the_train_paths(golden):
    g = golden('transforms')
    prm = np.stack([g['train%d_params' % s] for s in R.TRAIN_SEEDS])
    assert set(prm[:, 0]) == {0, 1} and set(prm[:, 1]) == {0, 1} and prm[:, 4].max() > 0 and prm[:, 5].max() > 0
    assert any(len(g['train%d_obox' % s]) < R.N_BOXES for s in R.TRAIN_SEEDS)


def test_descriptor_layouts_and_no_cpu_fallback():
    """the upload buffer's numpy records have the sizes of the C structs; CPU tensors fail loudly"""
    import torch
    from ood_object_detection_amd.effdet import preprocess as P
    assert np.dtype(P._DESC).itemsize == 64 and np.dtype(P._BOXP).itemsize == 48
    with pytest.raises(RuntimeError):
        P.resize_pad_batch([torch.zeros(4, 5, 3, dtype=torch.uint8)], 8)
