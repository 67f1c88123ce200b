"""Crops of detections on the device (csrc/pil_crop.hip, ppyolo_hip/crops.py, PilResizer(box=), Decode.crop_files) against the
installed Pillow, tests/golden/g26_pil_crops.npz and the numpy restatement tests/pil_crop_ref.py.  Array equality everywhere:
there is no tolerance."""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

import pil_crop_ref as cref
import pil_resize_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ('random', 'binary')
FILTER_IDS = dict(ids=lambda f: ref.NAMES[f])


@pytest.fixture(scope='module')
def g26():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'g26_pil_crops.npz'))


@pytest.fixture(scope='module')
def g25():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'g25_pil_resize.npz'))


@pytest.fixture(scope='module')
def resizers():
    from ppyolo_hip.resize import PilResizer
    return {f: PilResizer(f) for f in ref.FILTERS}


def pillow(img, ow, oh, f, box):
    return np.asarray(Image.fromarray(img).resize((ow, oh), f, box=tuple(float(v) for v in box)))


@pytest.mark.parametrize('f', ref.FILTERS, **FILTER_IDS)
def test_cases_equal_pillow_and_golden(resizers, g26, f):
    """Every shared case (fractional, integer, sub-pixel, border-touching and pass-skipping boxes, the 901-tap axis), both
    contents, through the list form.  The distinguishing case is in the list: a kernel that crops first fails here."""
    assert cref.DISTINGUISHING in cref.CASES
    for case in cref.CASES + [cref.TAPS_CASE]:
        (h, w), (ow, oh), box = case
        for kind in KINDS:
            img = cref.case_image(case, kind)
            out = resizers[f]([torch.from_numpy(img).cuda()], size=(ow, oh), box=[box])
            assert len(out) == 1 and out[0].is_cuda and out[0].dtype == torch.uint8 and tuple(out[0].shape) == (oh, ow, 3)
            got = out[0].cpu().numpy()
            assert np.array_equal(got, g26['%s_%s_f%d' % (cref.case_key(case), kind, f)]), (case, kind, 'golden')
            assert np.array_equal(got, pillow(img, ow, oh, f, box)), (case, kind, 'installed Pillow')


@pytest.mark.parametrize('f', ref.FILTERS, **FILTER_IDS)
def test_weights_parked_in_the_intermediate(resizers, f):
    """96 x 80 to 48 x 40: 8 (ow + oh) max(kx, ky) bytes fit in a crop's intermediate, so the plan kernel parks its double
    weights there instead of computing them twice (the small cases above mostly take the other route)."""
    from ppyolo_hip import ops
    h, w, ow, oh = 96, 80, 48, 40
    descs = ops.pil_crop_descs([(8, 3 * w, h, w)] * 2)
    ws_bytes, (kx, ky) = ops.pil_crop_plan_bytes(descs, 2, 1, 2, ow, oh, f)
    assert 8 * (ow + oh) * max(kx, ky) <= (h * ((3 * ow + 15) // 16 * 16) + 255) // 256 * 256
    imgs = [ref.content(h, w, kind, 90 + i) for i, kind in enumerate(KINDS)]
    for boxes in ([(0, 0, w, h), (3.25, 10.5, 71.75, 90.125)], [(20, 30, 21.5, 32), (0, 0, 80, 48)]):
        out = resizers[f]([torch.from_numpy(im).cuda() for im in imgs], size=(ow, oh), box=boxes)
        for im, b, t in zip(imgs, boxes, out):
            assert np.array_equal(t.cpu().numpy(), pillow(im, ow, oh, f, b)), (ref.NAMES[f], b)


def select_batch():
    """Three images of different sizes, the middle one a pitched view big[3:3+h, 5:5+w], and the hand-written rows."""
    host = [ref.content(h, w, KINDS[i & 1], 70 + i) for i, (h, w) in enumerate(cref.SELECT_SIZES)]
    h1, w1 = cref.SELECT_SIZES[1]
    big = torch.from_numpy(ref.content(h1 + 7, w1 + 9, 'random', 77)).cuda()
    host[1] = np.ascontiguousarray(big.cpu().numpy()[3:3 + h1, 5:5 + w1])
    dev = [torch.from_numpy(host[0]).cuda(), big[3:3 + h1, 5:5 + w1], host[2]]      # (the last one a numpy array: uploaded)
    assert not dev[1].is_contiguous()
    d, count = cref.select_rows_case()
    return host, dev, d, count


def expect_crops(host, d, count, thresh, pad, top_k, ow, oh, f):
    src, boxes = cref.select_rows(d, count, [im.shape[:2] for im in host], thresh, pad, top_k)
    crops = [cref.resize_box(host[i], ow, oh, f, b) for (i, _), b in zip(src, boxes)]
    return src, boxes, crops


@pytest.mark.parametrize('pad,top_k', [(0.0, None), (0.1, None), (0.0, 1), (0.25, 3)])
@pytest.mark.parametrize('f', ref.FILTERS, **FILTER_IDS)
def test_rows_batch_equals_restatement(f, pad, top_k):
    from ppyolo_hip.crops import DetectionCropper
    host, dev, d, count = select_batch()
    ow, oh = 12, 10
    cropper = DetectionCropper((ow, oh), filter=f, pad=pad, top_k=top_k)
    crops, src, total = cropper(dev, torch.from_numpy(d).cuda(), torch.from_numpy(count).cuda(), thresh=cref.SELECT_THRESH)
    n, K = d.shape[:2]
    assert crops.is_cuda and tuple(crops.shape) == (n * K, oh, ow, 3) and crops.dtype == torch.uint8
    assert tuple(src.shape) == (n * K, 2) and src.dtype == torch.int32 and tuple(total.shape) == (1,) and total.dtype == torch.int32
    want_src, want_boxes, want = expect_crops(host, d, count, cref.SELECT_THRESH, pad, top_k, ow, oh, f)
    t = int(total.cpu()[0])
    assert t == len(want_src) and t > 0
    assert src[:t].cpu().tolist() == [list(s) for s in want_src]
    assert (src[t:].cpu().numpy() == -1).all()
    assert np.array_equal(cropper.boxes[:t].cpu().numpy().view(np.uint32), np.array(want_boxes, np.float32).view(np.uint32))
    assert (cropper.boxes[t:].cpu().numpy() == 0).all()
    got = crops.cpu().numpy()
    for j, ((i, r), b) in enumerate(zip(want_src, want_boxes)):
        assert np.array_equal(got[j], want[j]), (i, r, 'restatement')
        assert np.array_equal(got[j], pillow(host[i], ow, oh, f, b)), (i, r, 'installed Pillow')
    assert not got[t:].any()
    # split: per image (rows, crops), views of the batch
    parts = cropper.split(crops, src, total)
    assert len(parts) == n
    at = 0
    for i, (rows, tens) in enumerate(parts):
        assert rows.tolist() == [r for (ii, r) in want_src if ii == i]
        assert tuple(tens.shape) == (len(rows), oh, ow, 3) and np.array_equal(tens.cpu().numpy(), got[at:at + len(rows)])
        at += len(rows)
    assert at == t


def test_all_rows_rejected():
    from ppyolo_hip.crops import DetectionCropper
    host, dev, d, count = select_batch()
    cropper = DetectionCropper((9, 7))
    for dd, cc, thresh in ((d, count, 2.0), (d, np.zeros(3, np.int32), 0.0), (np.full_like(d, np.nan), count, 0.0)):
        crops, src, total = cropper(dev, torch.from_numpy(dd).cuda(), torch.from_numpy(cc).cuda(), thresh=thresh)
        assert int(total.cpu()[0]) == 0 and not crops.cpu().numpy().any() and (src.cpu().numpy() == -1).all()
        assert [(len(r), tuple(t.shape)) for r, t in cropper.split(crops, src, total)] == [(0, (0, 7, 9, 3))] * 3


def test_one_image_without_rows():
    """count == 0 for the middle image of a batch: its neighbours' crops close ranks, split() gives it an empty group."""
    from ppyolo_hip.crops import DetectionCropper
    host, dev, d, count = select_batch()
    count = np.array([7, 0, 11], np.int32)
    cropper = DetectionCropper((12, 10), filter=ref.BICUBIC)
    crops, src, total = cropper(dev, torch.from_numpy(d).cuda(), torch.from_numpy(count).cuda(), thresh=cref.SELECT_THRESH)
    want_src, _, want = expect_crops(host, d, count, cref.SELECT_THRESH, 0.0, None, 12, 10, ref.BICUBIC)
    t = int(total.cpu()[0])
    assert t == len(want_src) == 10 and src[:t].cpu().tolist() == [list(s) for s in want_src]
    assert np.array_equal(crops[:t].cpu().numpy(), np.stack(want)) and not crops[t:].cpu().numpy().any()
    assert [len(rows) for rows, _ in cropper.split(crops, src, total)] == [2, 0, 8]


def test_two_runs_are_bit_identical():
    from ppyolo_hip.crops import DetectionCropper
    host, dev, d, count = select_batch()
    dd, cc = torch.from_numpy(d).cuda(), torch.from_numpy(count).cuda()
    for f in ref.FILTERS:
        cropper = DetectionCropper((31, 17), filter=f, pad=0.1)
        a = [t.clone() for t in cropper(dev, dd, cc, thresh=0.5)] + [cropper.boxes.clone()]
        b = list(cropper(dev, dd, cc, thresh=0.5)) + [cropper.boxes]
        assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('f', (ref.NEAREST, ref.BICUBIC, ref.LANCZOS), **FILTER_IDS)
def test_small_batch_after_a_large_one_reuses_the_workspace(f):
    """The tables and intermediates of the large call stay in the workspace: a small call on the same cropper must not read
    them (other strides, other taps per sample) and equals the same call on a fresh cropper."""
    from ppyolo_hip.crops import DetectionCropper
    host, dev, d, count = select_batch()
    used = DetectionCropper((12, 10), filter=f, pad=0.1)
    used(dev, torch.from_numpy(d).cuda(), torch.from_numpy(count).cuda(), thresh=0.0)
    small = ref.content(17, 23, 'random', 5)
    rows = np.array([[[1, 0.9, 2.5, 1.25, 20, 15.5], [0, 0.8, 0, 0, 23, 17], [3, 0.7, 7, 7, 7.5, 9]]], np.float32)
    cnt = np.array([3], np.int32)
    args = ([torch.from_numpy(small).cuda()], torch.from_numpy(rows).cuda(), torch.from_numpy(cnt).cuda())
    a = used(*args, thresh=0.0)
    ws_used = used._launcher._ws
    b = DetectionCropper((12, 10), filter=f, pad=0.1)(*args, thresh=0.0)
    assert used._launcher._ws is ws_used                      # the same workspace served both calls
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and int(a[2].cpu()[0]) == 3
    want = expect_crops([small], rows, cnt, 0.0, 0.1, None, 12, 10, f)[2]
    assert np.array_equal(a[0].cpu().numpy(), np.stack(want))


@pytest.mark.parametrize('f', ref.FILTERS, **FILTER_IDS)
def test_resizer_without_a_box_is_unchanged_and_the_full_box_equals_it(resizers, g25, f):
    for (h, w), (ow, oh) in ref.SMALL_CASES:
        for kind in KINDS:
            key = '%dx%d_%dx%d_%s' % (h, w, ow, oh, kind)
            img = torch.from_numpy(ref.content(h, w, kind, ref.case_seed(h, w, ow, oh))).cuda()
            want = g25['out_%s_f%d' % (key, f)]
            assert np.array_equal(resizers[f]([img], size=(ow, oh))[0].cpu().numpy(), want), (key, 'box=None')
            assert np.array_equal(resizers[f]([img], size=(ow, oh), box=None)[0].cpu().numpy(), want), (key, 'box=None')
            assert np.array_equal(resizers[f]([img], size=(ow, oh), box=[(0, 0, w, h)])[0].cpu().numpy(), want), (key, 'full box')


def test_resizer_box_batch_and_refusals(resizers):
    from ppyolo_hip._lib import PPYoloHipError
    host, dev, _, _ = select_batch()
    boxes = [(1.5, 2, 40.25, 33), (0, 0, 21, 33), (10, 20, 64, 63.5)]
    out = resizers[ref.HAMMING](dev, size=(14, 15), box=boxes)
    for im, b, t in zip(host, boxes, out):
        assert np.array_equal(t.cpu().numpy(), pillow(im, 14, 15, ref.HAMMING, b))
    with pytest.raises(PPYoloHipError) as e:
        resizers[ref.HAMMING](dev, size=(14, 15), box=[boxes[0], (0, 0, 21.5, 33), boxes[2]])
    assert 'image 1' in str(e.value) and '21.5' in str(e.value)
    tall = torch.zeros((301, 3, 3), dtype=torch.uint8, device='cuda')
    with pytest.raises(PPYoloHipError) as e:
        resizers[ref.HAMMING]([tall], size=(4, 4), box=[(0, 0, 3, 301)])
    assert 'taller than 100 x' in str(e.value)


def test_cropper_inputs_refused_by_name():
    from ppyolo_hip._lib import PPYoloHipError
    from ppyolo_hip.crops import DetectionCropper
    host, dev, d, count = select_batch()
    dd, cc = torch.from_numpy(d).cuda(), torch.from_numpy(count).cuda()
    cropper = DetectionCropper((8, 8))
    for args, word in (((dev, d, cc), 'dets'), ((dev, dd, count), 'count'), ((dev, dd.double(), cc), 'dets'), ((dev[:2], dd, cc), 'for 2 images'),
                       ((dev[:2] + [[1, 2]], dd, cc), 'image 2'), ((dev[:2] + [torch.zeros((4, 4, 3))], dd, cc), 'image 2')):
        with pytest.raises(PPYoloHipError) as e:
            cropper(*args)
        assert word in str(e.value), str(e.value)
    for kw, word in ((dict(size=(0, 4)), '0 x 4'), (dict(size=(8193, 4)), '8193'), (dict(size=(4, 4), pad=5), 'pad 5'),
                     (dict(size=(4, 4), top_k=0), 'top_k 0'), (dict(size=(4, 4), filter=9), 'filter=9')):
        with pytest.raises(PPYoloHipError) as e:
            DetectionCropper(**kw)(dev, dd, cc)
        assert word in str(e.value), str(e.value)
    assert int(cropper(dev, dd, cc, thresh=0.5)[2].cpu()[0]) == 12          # and it still works


# ---- the detector's own rows ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def detector():
    import jpeg_enc_cases as C
    import jpeg_fixtures as F
    from conftest import build_model
    from config import PPYOLO_r18vd_Config
    from model.decode_np import Decode
    cfg = PPYOLO_r18vd_Config()
    cfg.test_cfg['target_size'] = 64
    model, _ = build_model(cfg, 0, 'cuda')
    dec = Decode(model, ['c%d' % i for i in range(80)], True, cfg, for_test=True)
    return dec, model, [F.data(c[0]) for c in C.COCO]


def test_crops_of_the_models_own_rows_equal_pillow(detector):
    from ppyolo_hip.crops import DetectionCropper
    from ppyolo_hip.jpeg import JpegDecoder
    dec, model, files = detector
    images = JpegDecoder().decode(files)
    pimage, im_size = dec._preprocessor()(images)
    dets, count, _ = model.forward_padded(pimage, im_size)
    host = [im.cpu().numpy() for im in images]
    d, c = dets.cpu().numpy(), count.cpu().numpy()
    for f, pad, thresh in ((ref.BICUBIC, 0.0, 0.0), (ref.LANCZOS, 0.15, 0.0), (ref.BILINEAR, 0.05, float(np.median(d[0, :max(c[0], 1), 1])))):
        cropper = DetectionCropper((32, 24), filter=f, pad=pad)
        crops, src, total = cropper(images, dets, count, thresh=thresh)
        want_src, want_boxes, _ = expect_crops(host, d, c, thresh, pad, None, 32, 24, f)
        t = int(total.cpu()[0])
        assert t == len(want_src) and t > 0 and src[:t].cpu().tolist() == [list(s) for s in want_src]
        got = crops.cpu().numpy()
        for j, ((i, r), b) in enumerate(zip(want_src, want_boxes)):
            assert np.array_equal(got[j], pillow(host[i], 32, 24, f, b)), (ref.NAMES[f], i, r)
        assert not got[t:].any()


def test_crop_files_end_to_end(detector):
    """Decode.crop_files: per image the JPEG files of its detections, byte for byte JpegEncoder's encode of the crops the
    cropper cuts from the decoder's undrawn pixels; each decodes (JpegDecoder) to a 24 x 32 image."""
    from ppyolo_hip.crops import DetectionCropper
    from ppyolo_hip.jpeg import JpegDecoder, JpegEncoder
    dec, model, files = detector
    got_files, results = dec.crop_files(files, size=(32, 24), filter=ref.BICUBIC, pad=0.1, draw_thresh=0.0)
    images = JpegDecoder().decode(files)
    pimage, im_size = dec._preprocessor()(images)
    dets, count, _ = model.forward_padded(pimage, im_size)
    cropper = DetectionCropper((32, 24), filter=ref.BICUBIC, pad=0.1)
    parts = cropper.split(*cropper(images, dets, count, thresh=0.0))
    assert len(got_files) == len(results) == len(files) == 2
    n_files = 0
    for i, ((rows, tens), mine) in enumerate(zip(parts, got_files)):
        assert len(mine) == len(rows)
        if len(rows):
            assert mine == JpegEncoder().encode(list(tens.unbind(0))), i
            back = JpegDecoder().decode(mine[:2])
            assert all(tuple(b.shape) == (24, 32, 3) for b in back)
            assert all(Image.open(io.BytesIO(m)).size == (32, 24) for m in mine[:2])
        n_files += len(mine)
    assert n_files > 0
    want = dec.annotate_files(files, draw_thresh=2.0)[1]                       # (nothing drawn: the same rows)
    for (b, s, c), (wb, ws, wc) in zip(results, want):
        assert np.array_equal(b, wb) and np.array_equal(s, ws) and np.array_equal(c, wc)
