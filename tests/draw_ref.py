"""The drawing contract of ppyolo_hip.draw twice on the host: `paint`, a sequential numpy painter of
the rules as the kernel restates them, and `paint_pillow`, the same rows through Pillow's ImageDraw with its built-in bitmap
font -- the pin.  Both draw in place on a uint8 [h, w, 3] array, in memory order as it lies.

`paint` takes its glyphs from ppyolo_hip.label_font (the package's own table and paste model), so against the kernel it is
independent only as far as tests/test_draw_ref.py holds that table and model equal to the installed Pillow.  Those two tests
skip where Pillow has no load_default_imagefont; on such a machine the text comparison of tests/test_gpu_draw.py checks the
kernel against the package's own data, not against Pillow."""
import colorsys
import random

import numpy as np

from ppyolo_hip import label_font

TH = label_font.CELL_H
CW = label_font.CELL_W


def reference_colors(num_classes):
    """Reference model/decode_np.py:101-107 as written there, global generator and all."""
    hsv_tuples = [(1.0 * x / num_classes, 1., 1.) for x in range(num_classes)]
    colors = list(map(lambda x: colorsys.hsv_to_rgb(*x), hsv_tuples))
    colors = list(map(lambda x: (int(x[0] * 255), int(x[1] * 255), int(x[2] * 255)), colors))
    random.seed(0)
    random.shuffle(colors)
    random.seed(None)
    return colors


def colors_for(num_classes):
    state = random.getstate()
    try:
        return reference_colors(num_classes)
    finally:
        random.setstate(state)


def digits(score):
    """'d.dd' by the contract's rule: rint(float64(score) * 100), ties to even."""
    v = int(np.rint(np.float64(np.float32(score)) * 100.0))
    return '%d.%d%d' % (v // 100, v // 10 % 10, v % 10)


def drawn(row, thresh, num_classes):
    cls, score = np.float32(row[0]), np.float32(row[1])
    if not np.all(np.isfinite(np.asarray(row, np.float32))):
        return False
    return bool(score >= np.float32(thresh) and 0 <= cls < num_classes and 0 <= score <= 1)


def corners(row, h, w):
    def rnd(v):
        v = np.floor(np.float32(v) + np.float32(0.5))          # float32 sum and floor
        return int(min(max(v, np.float32(-2.0 ** 30)), np.float32(2.0 ** 30)))
    return max(0, rnd(row[2])), max(0, rnd(row[3])), min(w, rnd(row[4])), min(h, rnd(row[5]))


def _clip_fill(image, x0, y0, x1, y1, color):
    """Inclusive corners, x0 <= x1, y0 <= y1, clipped."""
    h, w = image.shape[:2]
    x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, w - 1), min(y1, h - 1)
    if x0 <= x1 and y0 <= y1:
        image[y0:y1 + 1, x0:x1 + 1] = color


def paint(image, rows, count, thresh, names, colors):
    h, w = image.shape[:2]
    rows = np.asarray(rows, np.float32).reshape(-1, 6)
    for r in range(min(int(count), len(rows))):
        row = rows[r]
        if not drawn(row, thresh, len(names)):
            continue
        cls = int(row[0])
        color = np.array(colors[cls], np.uint8)
        left, top, right, bottom = corners(row, h, w)
        xa, xb, ya, yb = min(left, right), max(left, right), min(top, bottom), max(top, bottom)
        _clip_fill(image, xa, ya, xb, ya, color)
        _clip_fill(image, xa, yb, xb, yb, color)
        _clip_fill(image, xa, ya, xa, yb, color)
        _clip_fill(image, xb, ya, xb, yb, color)
        label = names[cls] + ': ' + digits(row[1])
        tw = CW * len(label)
        _clip_fill(image, left, top - TH - 3, left + tw, top, color)
        band = label_font.text_mask([ord(c) for c in label])
        for v in range(TH):
            y = top - TH - 2 + v
            if not 0 <= y < h:
                continue
            for u in range(tw):
                if band[v][u] and 0 <= left + u < w:
                    image[y, left + u] = 0
    return image


def paint_pillow(image, rows, count, thresh, names, colors):
    """The same rows through Pillow.  Only for boxes whose rounded height is at least 1: Pillow's outline of a rectangle with
    top == bottom spills into the row below, which neither cv2 nor the contract does."""
    from PIL import Image, ImageDraw, ImageFont
    h, w = image.shape[:2]
    im = Image.fromarray(image, 'RGB')                # three bytes per pixel as they lie; no channel is interpreted
    d = ImageDraw.Draw(im)
    font = ImageFont.load_default_imagefont()
    rows = np.asarray(rows, np.float32).reshape(-1, 6)
    for r in range(min(int(count), len(rows))):
        row = rows[r]
        if not drawn(row, thresh, len(names)):
            continue
        cls = int(row[0])
        color = tuple(colors[cls])
        left, top, right, bottom = corners(row, h, w)
        assert top != bottom, 'Pillow cannot pin a flat outline'
        d.rectangle([min(left, right), min(top, bottom), max(left, right), max(top, bottom)], outline=color, width=1)
        label = '%s: %.2f' % (names[cls], row[1])
        label = ''.join(c if 32 <= ord(c) <= 126 else '?' for c in label)
        tw = CW * len(label)
        d.rectangle([left, top - TH - 3, left + tw, top], fill=color)
        d.text((left, top - TH - 2), label, fill=(0, 0, 0), font=font)
    image[...] = np.asarray(im)
    return image


# ---- seeded scenes ----------------------------------------------------------------------------------------------------------
NAMES = ['person', 'Nb', 'yA', 'traffic light', 'b', 'nAb', 'q', 'dog~', 'WWW', 'j', 'bicycle', 'A']


def scene(seed, flat=False):
    """(image, rows, count): an image 8..90 x 8..140, 1..13 boxes reaching 5 px outside every edge, reversed x corners, zero
    widths, right == w, bottom == h, labels cut by every edge, plenty of overlap; -1 padding rows after `count`.  The boxes
    are constructed so that bottom > top after rounding unless flat=True, which adds flat and thin boxes."""
    rng = np.random.RandomState(seed)
    h, w = int(rng.randint(8, 91)), int(rng.randint(8, 141))
    image = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    k = int(rng.randint(1, 14))
    rows = -np.ones((k + 2, 6), np.float32)
    for r in range(k):
        kind = rng.randint(0, 8)
        x0, x1 = rng.uniform(-5, w + 5, 2)
        if kind == 0:
            x0, x1 = max(x0, x1), min(x0, x1)          # reversed x corners
        elif kind == 1:
            x1 = x0                                     # zero width
        elif kind == 2:
            x1 = w + rng.uniform(-0.4, 5)               # right == w
        elif kind == 3:
            x0 = rng.uniform(-5, 0.4)                   # label cut by the left edge
        elif kind == 4:
            x0 = w - rng.uniform(0, 12)                 # label cut by the right edge
        # rounded top in [0, h - 1] after the clamp; rounded bottom strictly below it and at most h
        y0 = rng.uniform(-5, h - 1.6)
        top = max(0, int(np.floor(np.float32(y0) + np.float32(0.5))))
        y1 = rng.uniform(top + 1.0, h + 5)
        if kind == 5:
            y1 = h + rng.uniform(-0.4, 5)               # bottom == h
        elif kind == 6:
            y0 = rng.uniform(-5, 3)                     # label above the top edge
            top = max(0, int(np.floor(np.float32(y0) + np.float32(0.5))))
            y1 = rng.uniform(top + 1.0, h + 5)
        elif kind == 7:
            y0 = h - 1.6 - rng.uniform(0, 1)            # label at the bottom edge
            y1 = h + 1.0
        if flat and r % 3 == 0:
            y1 = y0                                     # top == bottom
        if flat and r % 3 == 1:
            x1 = x0                                     # left == right (with r % 3 == 0 and kind == 1: both)
        if flat and r == 5:
            x1, y1 = x0, y0
        rows[r] = (rng.randint(0, len(NAMES)), np.float32(rng.randint(0, 1001)) / np.float32(1000), x0, y0, x1, y1)
    if not flat:
        for r in range(k):
            c = corners(rows[r], h, w)
            assert c[3] > c[1], (seed, r, c)
    return image, rows, k


SCENES = 240          # how many seeds the CPU and the GPU test both run


def float32_ties():
    """Every (2k+1)/200 in [0, 1] that is a float32, and both float32 neighbours of every (2k+1)/200."""
    out = []
    for k in range(100):
        x = (2 * k + 1) / 200.0
        f = np.float32(x)
        if float(f) == x:
            out.append(f)
        out += [np.nextafter(f, np.float32(-1)), np.nextafter(f, np.float32(2))]
        if float(f) != x:
            out.append(f)
    return [v for v in out if 0 <= v <= 1]
