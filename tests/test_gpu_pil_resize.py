"""Pillow's resize on the device (csrc/pil_resize.hip, ppyolo_hip/resize.py, Preprocessor with use_cv2=False) against the
installed Pillow and tests/golden/g25_pil_resize.npz.  Array equality everywhere: there is no tolerance."""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

import pil_resize_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ('random', 'binary')
FILTER_IDS = dict(ids=lambda f: ref.NAMES[f])


@pytest.fixture(scope='module')
def g25():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'g25_pil_resize.npz'))


@pytest.fixture(scope='module')
def resizers():
    from ppyolo_hip.resize import PilResizer
    return {f: PilResizer(f) for f in ref.FILTERS}


def pillow(img, ow, oh, f):
    return np.asarray(Image.fromarray(img).resize((ow, oh), f))


def one(resizer, img, ow, oh):
    out = resizer([img], size=(ow, oh))
    assert len(out) == 1 and out[0].is_cuda and out[0].dtype == torch.uint8 and tuple(out[0].shape) == (oh, ow, 3)
    return out[0].cpu().numpy()


@pytest.mark.parametrize('f', ref.FILTERS, **FILTER_IDS)
def test_small_cases_equal_pillow_and_golden(resizers, g25, f):
    for (h, w), (ow, oh) in ref.SMALL_CASES:
        for kind in KINDS:
            key = '%dx%d_%dx%d_%s' % (h, w, ow, oh, kind)
            img = ref.content(h, w, kind, ref.case_seed(h, w, ow, oh))
            got = one(resizers[f], torch.from_numpy(img).cuda(), ow, oh)
            assert np.array_equal(got, g25['out_%s_f%d' % (key, f)]), (key, 'golden')
            assert np.array_equal(got, pillow(img, ow, oh, f)), (key, 'installed Pillow')


@pytest.mark.parametrize('f', ref.FILTERS, **FILTER_IDS)
def test_long_taps(resizers, f):
    """1080 x 1920 -> 64 x 64: lanczos reads 181 and 103 taps."""
    (h, w), (ow, oh) = ref.LONG_CASE
    for kind in KINDS:
        img = ref.content(h, w, kind, 3)
        assert np.array_equal(one(resizers[f], img, ow, oh), pillow(img, ow, oh, f)), kind      # (a numpy source: uploaded)


@pytest.mark.parametrize('f', (ref.BICUBIC, ref.LANCZOS), **FILTER_IDS)
def test_coco_size(resizers, f):
    (h, w), (ow, oh) = ref.COCO_CASE
    for kind in KINDS:
        img = ref.content(h, w, kind, 4)
        assert np.array_equal(one(resizers[f], torch.from_numpy(img).cuda(), ow, oh), pillow(img, ow, oh, f)), kind


@pytest.mark.parametrize('f', ref.FILTERS, **FILTER_IDS)
def test_source_is_a_view(resizers, f):
    """big[3:3+h, 5:5+w]: pixel stride 3, a row pitch and a start that are no multiple of 4 -- read where it lies."""
    for (h, w), (ow, oh) in ref.SMALL_CASES:
        big = torch.from_numpy(ref.content(h + 7, w + 9, 'random', 11)).cuda()
        view = big[3:3 + h, 5:5 + w]
        assert not view.is_contiguous() or h == 1
        got = one(resizers[f], view, ow, oh)
        assert np.array_equal(got, pillow(np.ascontiguousarray(big.cpu().numpy()[3:3 + h, 5:5 + w]), ow, oh, f)), (h, w, ow, oh)


@pytest.mark.parametrize('f', ref.FILTERS, **FILTER_IDS)
def test_one_batch_of_different_sizes(resizers, f):
    """Two-pass, horizontal-only, vertical-only and copy images in ONE call; device tensors and numpy arrays mixed."""
    sizes = [(37, 53), (13, 9), (16, 40), (40, 16), (16, 16)]
    imgs = [ref.content(h, w, KINDS[i & 1], 20 + i) for i, (h, w) in enumerate(sizes)]
    src = [torch.from_numpy(im).cuda() if i & 1 else im for i, im in enumerate(imgs)]
    for (ow, oh) in ((16, 16), (21, 10)):
        out = resizers[f](src, size=(ow, oh))
        assert len(out) == len(sizes)
        for im, t in zip(imgs, out):
            assert tuple(t.shape) == (oh, ow, 3)
            assert np.array_equal(t.cpu().numpy(), pillow(im, ow, oh, f)), (im.shape, ow, oh)


def test_two_runs_are_bit_identical(resizers):
    imgs = [torch.from_numpy(ref.content(h, w, 'random', 30 + h)).cuda() for h, w in ((240, 320), (187, 250), (64, 48))]
    for f in ref.FILTERS:
        a = [t.clone() for t in resizers[f](imgs, size=(96, 80))]
        b = resizers[f](imgs, size=(96, 80))
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_sources_and_sizes_refused_by_name(resizers):
    from ppyolo_hip._lib import PPYoloHipError
    r = resizers[ref.BICUBIC]
    good = torch.zeros((8, 8, 3), dtype=torch.uint8, device='cuda')
    rgba = torch.zeros((8, 8, 4), dtype=torch.uint8, device='cuda')
    for bad, word in ((torch.zeros((8, 8, 3), dtype=torch.uint8), 'cpu'), (good.float(), 'float32'), (good[:, :, :2], 'shape'),
                      (rgba[:, :, :3], 'strides'), (good.permute(1, 0, 2), 'strides'), ([[1, 2, 3]], 'list'),
                      (np.zeros((8, 8), np.uint8), 'numpy')):
        with pytest.raises(PPYoloHipError) as e:
            r([good, bad], size=(4, 4))
        assert 'image 1' in str(e.value) and word in str(e.value), str(e.value)
    for size, word in (((8193, 4), '8193'), ((4, 0), '4 x 0'), (5, 'size=5')):
        with pytest.raises(PPYoloHipError) as e:
            r([good], size=size)
        assert word in str(e.value)
    with pytest.raises(PPYoloHipError):
        r([], size=(4, 4))
    assert np.array_equal(r([good], size=(4, 4))[0].cpu().numpy(), np.zeros((4, 4, 3), np.uint8))      # and it still works


# ---- Preprocessor ---------------------------------------------------------------------------------------------------------------
def _cfg(**resize):
    from config import PPYOLO_2x_Config
    cfg = PPYOLO_2x_Config()
    cfg.resizeImage = dict(cfg.resizeImage, **resize)
    return cfg


def host_batch(cfg, images, S, f):
    """The reference's pipeline on the host with Pillow's pixels: normalisation_table applied to the resized image, transposed."""
    from ppyolo_hip.preprocess import normalisation_table
    n = cfg.normalizeImage
    lut = normalisation_table(n['mean'], n['std'], n.get('is_scale', True))
    out = np.empty((len(images), 3, S, S), np.float32)
    for i, im in enumerate(images):
        px = pillow(im, S, S, f)
        for c in range(3):
            out[i, c] = lut[c][px[:, :, 2 - c if cfg.decodeImage['to_rgb'] else c]]
    return out


@pytest.mark.parametrize('to_rgb', (True, False))
@pytest.mark.parametrize('f', ref.FILTERS, **FILTER_IDS)
def test_preprocessor_pil_mixed_batch(f, to_rgb):
    """Fails on the code before this path existed: that returned the cv2-cubic pixels whatever use_cv2 said."""
    from ppyolo_hip.preprocess import Preprocessor
    sizes = [(37, 53), (64, 48), (32, 32), (13, 9), (32, 50), (50, 32), (30, 30)]
    images = [ref.content(h, w, KINDS[i & 1], 40 + i) for i, (h, w) in enumerate(sizes)]
    for S in (32, 30):          # 16-byte stores, and the scalar tail of a size that is no multiple of 4
        cfg = _cfg(use_cv2=False, interp=f)
        cfg.decodeImage = dict(cfg.decodeImage, to_rgb=to_rgb)
        pre = Preprocessor(cfg, S)
        x, im_size = pre(images)
        assert x.is_cuda and x.dtype == torch.float32 and tuple(x.shape) == (len(images), 3, S, S)
        assert np.array_equal(im_size.cpu().numpy(), np.array(sizes, np.float32))
        want = host_batch(cfg, images, S, f)
        assert np.array_equal(x.cpu().numpy().view(np.uint32), want.view(np.uint32))
        x2, _ = pre(images[::-1])          # the staging buffer and the workspace are reused
        assert np.array_equal(x2.cpu().numpy().view(np.uint32), want[::-1].view(np.uint32))


def test_preprocessor_shipped_configuration_is_unchanged():
    """use_cv2 absent or True: the launch the parent ran, bit for bit (ops.preprocess_images is that launch)."""
    from config import PPYOLO_2x_Config
    from ppyolo_hip import ops
    from ppyolo_hip.preprocess import Preprocessor
    images = [ref.content(h, w, 'random', 60 + h) for h, w in ((120, 160), (94, 125), (160, 120), (33, 47))]
    for cfg in (PPYOLO_2x_Config(), _cfg(use_cv2=True)):
        pre = Preprocessor(cfg, 96)
        assert pre._pil is None
        x, _ = pre(images)
        want = torch.empty_like(x)
        ops.preprocess_images([torch.from_numpy(im).cuda() for im in images], 96, pre.lut, want, swap_rb=True)
        assert torch.equal(x.view(torch.int32), want.view(torch.int32))


def test_detect_files_is_pinned_to_pillow_end_to_end():
    """r18vd at 64 x 64, synthetic weights, the two COCO-sized JPEG files, use_cv2=False / interp=3: detect_files returns exactly
    the rows of model(x, im_size) with x built on the host from Pillow's decode, Pillow's resize and the reference's numpy
    normalisation -- every stage in front of the network is Pillow's, bit for bit."""
    import jpeg_enc_cases as C
    import jpeg_fixtures as F
    from conftest import build_model
    from config import PPYOLO_r18vd_Config
    from model.decode_np import Decode
    S = 64
    cfg = PPYOLO_r18vd_Config()
    cfg.test_cfg['target_size'] = S
    cfg.resizeImage = dict(cfg.resizeImage, use_cv2=False, interp=3)
    model, _ = build_model(cfg, 0, 'cuda')
    dec = Decode(model, ['c%d' % i for i in range(80)], True, cfg, for_test=True)
    files = [F.data(c[0]) for c in C.COCO]
    got = dec.detect_files(files)
    xs, sizes, bgr = [], [], []
    mean = np.array(list(cfg.normalizeImage['mean']))[np.newaxis, np.newaxis, :]
    std = np.array(list(cfg.normalizeImage['std']))[np.newaxis, np.newaxis, :]
    for data in files:
        rgb = np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))          # decodeImage to_rgb=True
        sizes.append([rgb.shape[0], rgb.shape[1]])
        bgr.append(torch.from_numpy(np.ascontiguousarray(rgb[:, :, ::-1])).cuda())
        im = np.asarray(Image.fromarray(rgb).resize((S, S), 3)).astype(np.float32, copy=False)
        im = im / 255.0                                                        # tools/transform.py:895-917
        im -= mean
        im /= std
        xs.append(im.transpose(2, 0, 1))                                       # :1052-1054
    x = torch.from_numpy(np.ascontiguousarray(np.stack(xs), dtype=np.float32)).cuda()
    preds = model(x, torch.tensor(sizes, dtype=torch.float32).cuda())
    assert len(got) == len(preds) == 2
    rows = 0
    for (boxes, scores, classes), p in zip(got, preds):
        wb, ws, wc = Decode._split(p.cpu().detach().numpy())
        assert boxes.shape == wb.shape and np.array_equal(boxes, wb) and np.array_equal(scores, ws) and np.array_equal(classes, wc)
        rows += len(ws)
    assert rows > 0
    # and the same files under the shipped configuration see other pixels: the switch is read
    cfg2 = PPYOLO_r18vd_Config()
    cfg2.test_cfg['target_size'] = S
    plain = Decode(model, ['c%d' % i for i in range(80)], True, cfg2, for_test=True)
    xa, _ = plain._preprocessor()(bgr)
    assert not torch.equal(xa, x)
