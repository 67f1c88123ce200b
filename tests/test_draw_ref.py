"""The drawing contract on the host (no GPU): the sequential painter of tests/draw_ref.py against Pillow's ImageDraw, the
committed font table against the installed Pillow, the digit rule against '%.2f', the colour tables against the
reference's lines."""
import os
import random
import sys

import numpy as np
import pytest

import draw_ref
from ppyolo_hip import label_font

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

SCENES = draw_ref.SCENES
float32_ties = draw_ref.float32_ties


def _has_imagefont():
    from PIL import ImageFont
    return hasattr(ImageFont, 'load_default_imagefont')


needs_imagefont = pytest.mark.skipif(not _has_imagefont(), reason='this Pillow has no ImageFont.load_default_imagefont')


@needs_imagefont
def test_painter_equals_pillow_on_every_scene():
    colors = draw_ref.colors_for(len(draw_ref.NAMES))
    boxes = 0
    seen = dict(reversed=0, zero_width=0, right_w=0, bottom_h=0, cut_left=0, cut_right=0, cut_top=0, overlap=0)
    for seed in range(SCENES):
        image, rows, count = draw_ref.scene(seed)
        h, w = image.shape[:2]
        a = draw_ref.paint(image.copy(), rows, count, 0.0, draw_ref.NAMES, colors)
        b = draw_ref.paint_pillow(image.copy(), rows, count, 0.0, draw_ref.NAMES, colors)
        assert np.array_equal(a, b), 'scene %d: %d pixels differ' % (seed, int((a != b).any(axis=2).sum()))
        boxes += count
        cs = [draw_ref.corners(r, h, w) for r in rows[:count]]
        for (l, t, r, b_), row in zip(cs, rows[:count]):
            tw = 6 * (len(draw_ref.NAMES[int(row[0])]) + 6)
            seen['reversed'] += r < l
            seen['zero_width'] += r == l
            seen['right_w'] += r == w
            seen['bottom_h'] += b_ == h
            seen['cut_left'] += l == 0
            seen['cut_right'] += l + tw >= w
            seen['cut_top'] += t - 14 < 0
        ext = [(min(l, r), t - 14, max(l, r, l + 6 * (len(draw_ref.NAMES[int(row[0])]) + 6)), max(t, b_))
               for (l, t, r, b_), row in zip(cs, rows[:count])]             # box and label of each row
        seen['overlap'] += any(p[0] <= q[2] and q[0] <= p[2] and p[1] <= q[3] and q[1] <= p[3]
                               for i, p in enumerate(ext) for q in ext[:i])
    assert boxes >= 1200
    assert all(v >= 20 for v in seen.values()), seen


@needs_imagefont
def test_font_table_is_what_the_tool_extracts():
    import make_label_font
    rects, bitmaps = make_label_font.extract()
    assert tuple(rects) == label_font.RECTS
    assert tuple(bitmaps) == label_font.BITMAPS
    assert make_label_font.render(rects, bitmaps) == open(make_label_font.OUT).read()
    assert sum(r[0] == -1 for r in rects) == 29
    assert len(label_font.device_table()) == 95 * 16


@needs_imagefont
def test_paste_model_equals_getmask():
    from PIL import ImageFont
    font = ImageFont.load_default_imagefont()
    rng = random.Random(7)
    for _ in range(1500):
        s = ''.join(chr(rng.randint(32, 126)) for _ in range(rng.randint(1, 24)))
        m = font.getmask(s)
        assert m.size == (6 * len(s), 11)
        ref = (np.frombuffer(bytes(m), np.uint8).reshape(11, -1) != 0).astype(np.uint8)
        assert np.array_equal(np.array(label_font.text_mask([ord(c) for c in s]), np.uint8), ref), s


def test_unknown_characters_are_question_marks():
    assert label_font.glyph(7) == label_font.glyph(ord('?')) == label_font.glyph(200)
    assert label_font.text_mask([0x4e2d]) == label_font.text_mask([ord('?')])


def test_digits_equal_percent_2f():
    ties = float32_ties()
    assert sum(float(t) * 200 % 2 == 1 for t in ties) >= 3          # 0.125, 0.375, ... are float32
    for v in ties + [np.float32(0), np.float32(1), np.float32(0.005), np.float32(0.995)]:
        assert draw_ref.digits(v) == '%.2f' % v, float(v)
    rng = np.random.RandomState(0)
    for v in rng.random_sample(20000).astype(np.float32):
        assert draw_ref.digits(v) == '%.2f' % v, float(v)


@needs_imagefont
def test_pillow_flat_outline_quirk():
    """The one place the contract leaves Pillow: its outline of a height-zero rectangle also sets pixels in the row below.
    The contract's (and cv2's) is one row.  Pinned as observed, so a Pillow that changes it is noticed here."""
    from PIL import Image, ImageDraw
    image = np.zeros((12, 40, 3), np.uint8)
    rows = np.array([[0, 0.5, 3, 8, 20, 8]], np.float32)
    a = draw_ref.paint(image.copy(), rows, 1, 0.0, ['x'], [(9, 9, 9)])
    assert (a[9:] == 0).all() and (a[8, 3:21] != 0).all()                   # the contract: one row
    im = Image.fromarray(image.copy(), 'RGB')
    ImageDraw.Draw(im).rectangle([3, 8, 20, 8], outline=(9, 9, 9), width=1)
    b = np.asarray(im)
    one_row = np.zeros_like(image)
    one_row[8, 3:21] = 9
    assert np.array_equal(b[:9], one_row[:9])                               # row 8 is the outline everybody draws
    assert (b[9] != 0).any() and (b[10:] == 0).all()                        # the quirk: extra pixels in the row below, only there
