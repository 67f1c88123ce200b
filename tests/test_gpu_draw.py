"""csrc/draw.hip on the GPU, bit for bit against the sequential painter of tests/draw_ref.py (which test_draw_ref.py pins to
Pillow): scenes, flat and thin boxes, painter's order, skipped rows, addressing, the digits, and the Decode entry points."""
import io

import numpy as np
import pytest
import torch

import draw_ref
from draw_ref import SCENES, float32_ties

pytestmark = pytest.mark.gpu

NAMES = draw_ref.NAMES
COLORS = draw_ref.colors_for(len(NAMES))
_DRAWERS = {}


def drawer(names=NAMES):
    from ppyolo_hip.draw import BoxDrawer
    key = tuple(names)
    if key not in _DRAWERS:
        _DRAWERS[key] = BoxDrawer(list(names))
    return _DRAWERS[key]


def pad(rows_list, k=None):
    k = k or max(len(r) for r in rows_list)
    dets = -np.ones((len(rows_list), k, 6), np.float32)
    for i, r in enumerate(rows_list):
        dets[i, :len(r)] = r
    return dets


def draw_batch(images, rows_list, counts, thresh=0.0, names=NAMES, k=None):
    """Numpy images -> what the kernel makes of them (one launch)."""
    dev = [torch.from_numpy(im).cuda() for im in images]
    dets = torch.from_numpy(pad(rows_list, k)).cuda()
    out = drawer(names)(dev, dets, torch.tensor(counts, dtype=torch.int32).cuda(), thresh)
    assert all(a is b for a, b in zip(out, dev))
    return [t.cpu().numpy() for t in dev]


def expect(images, rows_list, counts, thresh=0.0, names=NAMES, colors=COLORS):
    return [draw_ref.paint(im.copy(), r, c, thresh, names, colors) for im, r, c in zip(images, rows_list, counts)]


def same(got, want):
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and np.array_equal(a, b), 'image %d: %d pixels differ' % (i, int((a != b).any(axis=2).sum()))


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason='needs two visible devices')
def test_another_cards_memory_is_refused_by_every_object_built_with_an_unindexed_device():
    """hostio.same_device: 'cuda' is the current device, so a tensor on cuda:1 is refused while device 0 is current, not read or
    drawn on from device 0's stream."""
    from ppyolo_hip._lib import PPYoloHipError
    from ppyolo_hip.jpeg import JpegEncoder
    from ppyolo_hip.resize import BICUBIC, PilResizer
    assert torch.cuda.current_device() == 0
    far = torch.zeros((8, 9, 3), dtype=torch.uint8, device='cuda:1')
    dets, count = torch.zeros((1, 1, 6), device='cuda'), torch.zeros((1,), dtype=torch.int32, device='cuda')
    for call in (lambda: PilResizer(BICUBIC, 'cuda')([far], size=(4, 4)), lambda: drawer()([far], dets, count),
                 lambda: JpegEncoder(device='cuda').encode([far])):
        with pytest.raises(PPYoloHipError, match='image 0: lives on cuda:1'):
            call()


def test_seeded_scenes_in_one_batch():
    scenes = [draw_ref.scene(s) for s in range(SCENES)]
    images, rows, counts = [s[0] for s in scenes], [s[1] for s in scenes], [s[2] for s in scenes]
    same(draw_batch(images, rows, counts), expect(images, rows, counts))


def test_flat_and_thin_boxes():
    scenes = [draw_ref.scene(1000 + s, flat=True) for s in range(48)]
    images, rows, counts = [s[0] for s in scenes], [s[1] for s in scenes], [s[2] for s in scenes]
    # and the three by hand: top == bottom, left == right, both
    images.append(np.full((30, 90, 3), 7, np.uint8))
    rows.append(np.array([[0, 0.5, 5, 20, 60, 20], [1, 0.25, 70, 16, 70, 28], [2, 1.0, 40, 8.2, 40.3, 7.6]], np.float32))
    counts.append(3)
    want = expect(images, rows, counts)
    assert (want[-1][20, 5:61] == COLORS[0]).all() and (want[-1][21, 5:61] == 7).all()          # one row, nothing below it
    same(draw_batch(images, rows, counts), want)


def test_box_wholly_outside():
    image = np.random.RandomState(3).randint(0, 256, (40, 70, 3)).astype(np.uint8)
    rows = [np.array([[0, 0.9, -500, -400, -300, -200]], np.float32), np.array([[1, 0.9, 300, 200, 500, 400]], np.float32),
            np.array([[2, 0.9, 3e9, 3e9, 4e9, 4e9]], np.float32), np.array([[3, 0.9, -4e9, -4e9, -3e9, -3e9]], np.float32),
            np.array([[4, 0.9, 10, 300, 30, 400]], np.float32)]
    images = [image.copy() for _ in rows]
    same(draw_batch(images, rows, [1] * len(rows)), expect(images, rows, [1] * len(rows)))


def _overlapping(k, size, seed):
    rng = np.random.RandomState(seed)
    image = rng.randint(0, 256, (size, size, 3)).astype(np.uint8)
    rows = np.zeros((k, 6), np.float32)
    rows[:, 0] = rng.randint(0, len(NAMES), k)
    rows[:, 1] = rng.randint(0, 1001, k) / np.float32(1000)
    rows[:, 2] = rng.uniform(-2, size * 0.4, k)
    rows[:, 3] = rng.uniform(-2, size * 0.4, k)
    rows[:, 4] = rows[:, 2] + rng.uniform(size * 0.5, size, k)          # every box spans the centre: all overlap
    rows[:, 5] = rows[:, 3] + rng.uniform(size * 0.5, size, k)
    return image, rows


@pytest.mark.parametrize('k,size', [(100, 64), (1024, 32)])
def test_painters_order(k, size):
    image, rows = _overlapping(k, size, k)
    want = expect([image], [rows], [k])
    a = draw_batch([image.copy()], [rows], [k])
    b = draw_batch([image.copy()], [rows], [k])
    assert np.array_equal(a[0], b[0])
    same(a, want)


def test_skipped_rows_leave_every_other_pixel_alone():
    rng = np.random.RandomState(5)
    image = rng.randint(0, 256, (60, 120, 3)).astype(np.uint8)
    C = len(NAMES)
    rows = np.array([[0, 0.50, 5, 20, 40, 50],            # drawn
                     [1, 0.29999, 50, 20, 90, 50],        # below draw_thresh
                     [2, 0.30, 20, 30, 70, 55],           # exactly at it: drawn
                     [3, 0.9, np.nan, 20, 90, 50],        # NaN coordinate
                     [4, 0.9, 10, 20, np.inf, 50],        # infinite coordinate
                     [C, 0.9, 10, 20, 90, 50],            # class C
                     [-1, 0.9, 10, 20, 90, 50],           # class -1
                     [5, 1.5, 10, 20, 90, 50],            # score above 1
                     [5, np.nan, 10, 20, 90, 50],         # NaN score
                     [-1, -1, -1, -1, -1, -1],            # the padding row
                     [6, 0.8, 60, 18, 110, 40],           # drawn, after skipped ones
                     [7, 0.99, 0, 0, 119, 59]],           # past count: never drawn
                    np.float32)
    thresh = float(np.float32(0.30))
    images = [image.copy(), image.copy(), image.copy()]
    rl, counts = [rows, rows, rows[:3]], [11, 0, 3]
    got, want = draw_batch(images, rl, counts, thresh, k=16), expect(images, rl, counts, thresh)
    same(got, want)
    assert np.array_equal(got[1], image)                                                   # count = 0: untouched
    only = draw_ref.paint(image.copy(), rows[[0, 2, 10]], 3, 0.0, NAMES, COLORS)
    assert np.array_equal(got[0], only)                                                    # exactly rows 0, 2 and 10
    assert (got[0] != image).any() and (got[0] == image).all(axis=2).sum() > 1000


def test_addressing_crop_odd_base_and_unit_sizes():
    rng = np.random.RandomState(9)
    big = rng.randint(0, 256, (80, 150, 3)).astype(np.uint8)
    flat = rng.randint(0, 256, (1 + 41 * 133 + 64,)).astype(np.uint8)
    tall, wide, one = [rng.randint(0, 256, s).astype(np.uint8) for s in ((50, 1, 3), (1, 70, 3), (1, 1, 3))]
    d_big, d_flat = torch.from_numpy(big).cuda(), torch.from_numpy(flat).cuda()
    crop = d_big[3:3 + 60, 5:5 + 100]                                            # pitched view
    odd = d_flat[1:].as_strided((41, 43, 3), (133, 3, 1))                        # odd base, odd pitch
    assert crop.data_ptr() % 2 == 1 and odd.data_ptr() % 2 == 1 and not crop.is_contiguous()
    dev = [crop, odd, torch.from_numpy(tall).cuda(), torch.from_numpy(wide).cuda(), torch.from_numpy(one).cuda()]
    rows = [np.array([[0, 0.5, -3, 10, 104, 70], [3, 0.7, 40, 0, 99.6, 59.6]], np.float32),
            np.array([[1, 0.5, 2, 16, 30, 35], [2, 0.7, 20, 2, 50, 45]], np.float32),
            np.array([[4, 0.5, 0, 20, 0.4, 40], [5, 0.7, -2, 3, 3, 60]], np.float32),
            np.array([[6, 0.5, 10, 0, 40, 0.4], [7, 0.7, 30, -3, 90, 3]], np.float32),
            np.array([[8, 0.5, 0, 0, 0.2, 0.2], [9, 0.7, -1, -1, 2, 2]], np.float32)]
    hosts = [t.cpu().numpy().copy() for t in dev]
    drawer()(dev, torch.from_numpy(pad(rows)).cuda(), torch.tensor([2] * 5, dtype=torch.int32).cuda())
    same([t.cpu().numpy() for t in dev], expect(hosts, rows, [2] * 5))
    # the surroundings of the views are as they were
    after_big, after_flat = d_big.cpu().numpy(), d_flat.cpu().numpy()
    keep = np.ones(big.shape[:2], bool)
    keep[3:63, 5:105] = False
    assert np.array_equal(after_big[keep], big[keep]) and (after_big[~keep] != big[~keep]).any()
    inside = np.zeros(flat.shape, bool)
    for y in range(41):
        inside[1 + 133 * y:1 + 133 * y + 129] = True
    assert np.array_equal(after_flat[~inside], flat[~inside]) and (after_flat[inside] != flat[inside]).any()


def test_digits_on_the_device_are_percent_2f():
    scores = float32_ties() + [np.float32(0), np.float32(1), np.float32(0.005), np.float32(0.995)]
    images = [np.full((20, 64, 3), 200, np.uint8) for _ in scores]
    rows = [np.array([[11, s, 2, 15, 60, 19]], np.float32) for s in scores]
    got = draw_batch(images, rows, [1] * len(scores))
    from PIL import ImageFont
    paint = draw_ref.paint_pillow if hasattr(ImageFont, 'load_default_imagefont') else draw_ref.paint
    want = [paint(im.copy(), r, 1, 0.0, NAMES, COLORS) for im, r in zip(images, rows)]          # Pillow prints '%.2f' itself
    same(got, want)
    assert len({w.tobytes() for w in want}) >= 100                                               # the labels do differ


def _decode(size):
    from conftest import build_model
    from config import PPYOLO_r18vd_Config
    from model.decode_np import Decode
    cfg = PPYOLO_r18vd_Config()
    cfg.test_cfg['target_size'] = size
    model, _ = build_model(cfg, 0, 'cuda')
    names = [(NAMES[i % len(NAMES)] + str(i))[:20] for i in range(80)]
    return Decode(model, names, True, cfg, for_test=True), names, cfg


def test_detect_image_and_detect_batch_draw_in_place():
    from ppyolo_hip import synth
    dec, names, cfg = _decode(64)
    colors = draw_ref.colors_for(80)
    assert dec.drawer().colors == colors
    x = synth.synth_images(2, 64).numpy()
    ims = np.array([[48, 64], [64, 40]], dtype=np.int32)
    rng = np.random.RandomState(1)
    images = [rng.randint(0, 256, (48, 64, 3)).astype(np.uint8), rng.randint(0, 256, (64, 40, 3)).astype(np.uint8)]
    plain = dec.detect_image(images[0].copy(), x[:1], ims[:1], draw_image=False)
    for thresh in (0.0, float(np.median(plain[2])) if len(plain[2]) else 0.5):
        image = images[0].copy()
        out, boxes, scores, classes = dec.detect_image(image, x[:1], ims[:1], draw_image=True, draw_thresh=thresh)
        assert out is image
        for a, b in zip((boxes, scores, classes), plain[1:]):
            assert np.array_equal(a, b)                                       # the results are what draw_image=False returns
        assert len(scores) > 0
        pos = scores >= thresh
        rows = np.concatenate([classes[pos, None].astype(np.float32), scores[pos, None], boxes[pos]], axis=1)
        assert np.array_equal(image, draw_ref.paint(images[0].copy(), rows, len(rows), 0.0, names, colors))
        assert not np.array_equal(image, images[0])
    batch = [im.copy() for im in images]
    out, bb, ss, cc = dec.detect_batch(batch, x, ims, draw_image=True, draw_thresh=0.0)
    for i in range(2):
        assert out[i] is batch[i]
        rows = np.concatenate([cc[i][:, None].astype(np.float32), ss[i][:, None], bb[i]], axis=1)
        assert np.array_equal(batch[i], draw_ref.paint(images[i].copy(), rows, len(rows), 0.0, names, colors))
    # Decode.draw with the reference's signature, on a device tensor as well
    t = torch.from_numpy(images[0]).cuda()
    assert dec.draw(t, bb[0], ss[0], cc[0]) is t and np.array_equal(t.cpu().numpy(), batch[0])
    empty = images[1].copy()
    assert dec.draw(empty, np.array([]), np.array([]), np.array([])) is empty and np.array_equal(empty, images[1])


def test_annotate_files_equals_pillow_end_to_end():
    from PIL import Image
    import jpeg_enc_cases as C
    import jpeg_fixtures as F
    dec, names, cfg = _decode(320)
    colors = draw_ref.colors_for(80)
    cfg.test_cfg['draw_thresh'] = 0.02
    files_in = [F.data(c[0]) for c in C.COCO]
    files, results = dec.annotate_files(files_in)                            # draw_thresh=None: the configuration's
    plain = dec.detect_files(files_in)
    assert len(files) == len(results) == 2
    drawn = 0
    for data, got, (boxes, scores, classes), ref in zip(files_in, files, results, plain):
        for a, b in zip((boxes, scores, classes), ref):
            assert a.shape == b.shape and np.array_equal(a, b)
        bgr = np.ascontiguousarray(np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))[:, :, ::-1])
        rows = np.concatenate([classes[:, None].astype(np.float32), scores[:, None], boxes], axis=1) if len(scores) else np.zeros((0, 6), np.float32)
        drawn += int((rows[:, 1] >= np.float32(0.02)).sum())
        draw_ref.paint(bgr, rows, len(rows), 0.02, names, colors)
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(buf, 'JPEG', quality=95, subsampling='4:2:0')
        assert got == buf.getvalue()
    assert drawn > 0
    files0, _ = dec.annotate_files(files_in, draw_thresh=2.0)                # nothing reaches the threshold: the plain re-encode
    assert all(C.matches_coco(c[0], f) for c, f in zip(C.COCO, files0))
