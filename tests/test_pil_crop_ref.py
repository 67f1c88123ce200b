"""Pillow's resize(box=), host side (no GPU, no library): the numpy restatement (tests/pil_crop_ref.py) equals the installed
Pillow and tests/golden/g26_pil_crops.npz on the shared cases and on a seeded sweep, and the select rule does what its
hand-written rows say.  Pillow is imported plainly: without it the pin fails, it does not skip."""
import os

import numpy as np
import pytest
from PIL import Image

import pil_crop_ref as cref
import pil_resize_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ('random', 'binary')
f32 = np.float32


@pytest.fixture(scope='module')
def g26():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'g26_pil_crops.npz'))


def pillow(img, ow, oh, f, box):
    return np.asarray(Image.fromarray(img).resize((ow, oh), f, box=tuple(float(v) for v in box)))


@pytest.mark.parametrize('case', cref.CASES + [cref.TAPS_CASE], ids=cref.case_key)
def test_restatement_equals_pillow_and_golden(case, g26):
    (h, w), (ow, oh), box = case
    for kind in KINDS:
        img = cref.case_image(case, kind)
        for f in ref.FILTERS:
            got = cref.resize_box(img, ow, oh, f, box)
            assert got.shape == (oh, ow, 3)
            assert np.array_equal(got, g26['%s_%s_f%d' % (cref.case_key(case), kind, f)]), (case, ref.NAMES[f], 'golden')
            assert np.array_equal(got, pillow(img, ow, oh, f, box)), (case, ref.NAMES[f], 'installed Pillow')


def test_taps_case_reads_901_taps():
    (h, w), (ow, oh), box = cref.TAPS_CASE
    assert cref.axis_table_box(w, box[0], box[2], ow, ref.LANCZOS)[0] == 901


def test_restatement_sweep():
    """300 seeded cases beyond the shared list, all six filters, content alternating random / binary."""
    for i, case in enumerate(cref.seeded_cases(seed=2600, count=300)):
        (h, w), (ow, oh), box = case
        img = ref.content(h, w, KINDS[i & 1], 5000 + i)
        for f in ref.FILTERS:
            assert np.array_equal(cref.resize_box(img, ow, oh, f, box), pillow(img, ow, oh, f, box)), (case, ref.NAMES[f])


def test_integer_box_is_not_crop_then_resize():
    """The clamp is to the image, not to the box: resize(box=(4, 3, 20, 15)) reads the pixels around the box.  A restatement (or
    a kernel) that crops first cannot pass the case list, because this case is in it."""
    case = cref.DISTINGUISHING
    (h, w), (ow, oh), box = case
    assert case in cref.CASES
    img = cref.case_image(case, 'random')
    x0, y0, x1, y1 = box
    for f in (ref.BICUBIC, ref.LANCZOS, ref.BILINEAR, ref.HAMMING):
        with_box = pillow(img, ow, oh, f, box)
        cropped = np.asarray(Image.fromarray(img).crop(box).resize((ow, oh), f))
        assert not np.array_equal(with_box, cropped), ref.NAMES[f]
        assert np.array_equal(cref.resize_box(img, ow, oh, f, box), with_box)
        assert np.array_equal(ref.resize(np.ascontiguousarray(img[y0:y1, x0:x1]), ow, oh, f), cropped)
    d = np.abs(pillow(img, ow, oh, ref.BICUBIC, box).astype(int)
               - np.asarray(Image.fromarray(img).crop(box).resize((ow, oh), ref.BICUBIC)).astype(int)).max()
    assert d >= 5, d


def test_box_is_rounded_to_float32():
    """Pillow parses the box with "(ffff)": a double that is no float32 is rounded first, and the subtraction is float32's."""
    img = ref.content(40, 64, 'random', 9)
    box = (0.1, 0.2, 63.9 + 1e-9, 39.7)
    for f in ref.FILTERS:
        assert np.array_equal(cref.resize_box(img, 13, 11, f, box), pillow(img, 13, 11, f, box))
    assert cref.axis_scale(0.1, 63.9, 13) != (63.9 - 0.1) / 13


def test_pillow_refuses_what_the_rule_says():
    im = Image.fromarray(ref.content(10, 12, 'random', 1))
    for box in ((-0.5, 0, 5, 5), (0, -1, 5, 5), (0, 0, 12.5, 5), (0, 0, 5, 10.25)):
        with pytest.raises(ValueError):
            im.resize((4, 4), 3, box=box)
    im.resize((4, 4), 3, box=(3, 3, 3, 3))          # an empty box is accepted


# ---- the select rule ------------------------------------------------------------------------------------------------------------
def test_select_rows_hand_written():
    d, count = cref.select_rows_case()
    src, boxes = cref.select_rows(d, count, cref.SELECT_SIZES, cref.SELECT_THRESH, 0.0)
    assert src == [(0, 0), (0, 5), (1, 0), (1, 1)] + [(2, r) for r in range(8)]
    assert [tuple(float(v) for v in b) for b in boxes[:4]] == [(10, 5, 30, 25), (1.5, 12, 30, 39.5), (0, 0, 21, 33), (2.5, 3.5, 8.25, 30)]


def test_select_rows_score_equal_to_thresh_is_taken():
    d, count = cref.select_rows_case()
    assert (0, 0) in cref.select_rows(d, count, cref.SELECT_SIZES, 0.5, 0.0)[0]
    assert (0, 0) not in cref.select_rows(d, count, cref.SELECT_SIZES, float(np.nextafter(f32(0.5), f32(1))), 0.0)[0]


def test_select_rows_top_k_count_zero_and_garbage():
    d, count = cref.select_rows_case()
    src, _ = cref.select_rows(d, count, cref.SELECT_SIZES, cref.SELECT_THRESH, 0.0, top_k=1)
    assert src == [(0, 0), (1, 0), (2, 0)]
    src, _ = cref.select_rows(d, np.array([7, 0, 11]), cref.SELECT_SIZES, cref.SELECT_THRESH, 0.0)
    assert [s for s in src if s[0] == 1] == []
    assert np.isnan(d[0, 7]).any() and np.isnan(d[1, 2:]).any()          # the rows behind count hold NaN garbage
    src, _ = cref.select_rows(d, np.array([0, 0, 0]), cref.SELECT_SIZES, 0.0, 0.0)
    assert src == []


def test_select_rows_pad_is_clipped_at_two_borders():
    d, count = cref.select_rows_case()
    src, boxes = cref.select_rows(d, count, cref.SELECT_SIZES, cref.SELECT_THRESH, 0.1)
    b = boxes[src.index((0, 5))]
    bw, bh = f32(30) - f32(1.5), f32(39.5) - f32(12)
    assert b == (f32(0), f32(12) - f32(0.1) * bh, f32(30) + f32(0.1) * bw, f32(40))
    assert all(type(v) is np.float32 for v in b)
    assert boxes[src.index((1, 0))] == (0, 0, 21, 33)                   # the whole image stays the whole image


def test_select_list_keeps_order_and_skips_invalid():
    sizes = [(10, 12), (20, 8)]
    boxes = [(0, 0, 8, 20), (1, 1, 5, 5), (1, 1, 13, 5), (2, 2, 2, 9), (0, 0, 4, 4), (0, 0, 4, 4)]
    image = [1, 0, 0, 1, 2, -1]
    src, got = cref.select_list(boxes, image, sizes)
    assert src == [(1, 0), (0, 1)] and got == [(0, 0, 8, 20), (1, 1, 5, 5)]
