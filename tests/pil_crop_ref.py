"""Pillow's `Image.resize((ow, oh), filter, box=(x0, y0, x1, y1))` for 3-channel uint8 images, restated in numpy on top of
tests/pil_resize_ref.py, and the select rule of the crop kernels (csrc/pil_crop.hip).  Every float of
the tables is a Python float (an IEEE double, one rounding per operation, in Pillow's order); the box is four float32, and
the one float32 operation of the rule -- `in1 - in0` -- is done in numpy's float32.

tests/test_pil_crop_ref.py pins this file to the installed Pillow and to tests/golden/g26_pil_crops.npz;
tests/test_gpu_pil_crop.py pins the kernels to this file and to both."""
import math

import numpy as np

import pil_resize_ref as ref

f32 = np.float32


def box32(box):
    """The box as Pillow's C sees it: "(ffff)" rounds every value to float32."""
    return tuple(f32(v) for v in box)


def axis_scale(in0, in1, outsz):
    return float(f32(in1) - f32(in0)) / outsz          # the subtraction in float32, the division in double


def axis_table_box(insz, in0, in1, outsz, f):
    """Filters 1..5, one axis with a box [in0, in1): (ksize, bounds int32 [out, 2] = (xmin, count), k int32 [out, ksize]).  The
    taps are clamped to the IMAGE (0..insz), not to the box."""
    fn = ref._FUNCS[f]
    in0 = float(f32(in0))
    scale = axis_scale(in0, in1, outsz)
    fs = max(scale, 1.0)
    support = ref.SUPPORT[f] * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    bounds = np.zeros((outsz, 2), np.int32)
    k = np.zeros((outsz, ksize), np.int32)
    for xx in range(outsz):
        center = in0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), insz) - xmin
        w = [fn((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[xx] = (xmin, xmax)
        for x, v in enumerate(w):
            k[xx, x] = int(-0.5 + v * (1 << ref.PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << ref.PRECISION_BITS))
    return ksize, bounds, k


def nearest_map_box(in0, in1, outsz):
    """NEAREST, one axis: the coordinate starts at in0 + step / 2 and is accumulated by repeated addition."""
    step = axis_scale(in0, in1, outsz)
    xo = float(f32(in0)) + step * 0.5
    idx = np.zeros(outsz, np.int32)
    for x in range(outsz):
        idx[x] = int(math.floor(xo))
        xo += step
    return idx


def resize_box(img, ow, oh, f, box):
    """uint8 [h, w, 3] -> uint8 [oh, ow, 3], as Image.fromarray(img).resize((ow, oh), f, box=box)."""
    img = np.ascontiguousarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
    h, w = img.shape[:2]
    x0, y0, x1, y1 = box32(box)
    assert 0 <= x0 and 0 <= y0 and x1 <= w and y1 <= h and x0 <= x1 and y0 <= y1, 'Pillow refuses this box'
    need_h = ow != w or x0 != 0 or x1 != ow
    need_v = oh != h or y0 != 0 or y1 != oh
    if not need_h and not need_v:
        return img.copy()
    if f == ref.NEAREST:
        return np.ascontiguousarray(img[nearest_map_box(y0, y1, oh)][:, nearest_map_box(x0, x1, ow)])
    kv, bv, cv = axis_table_box(h, y0, y1, oh, f)
    first, last = int(bv[0, 0]), int(bv[oh - 1, 0] + bv[oh - 1, 1])
    if need_h:
        img = ref._pass(img[first:last], axis_table_box(w, x0, x1, ow, f), 1)      # only the rows the vertical taps read
        bv = bv.copy()
        bv[:, 0] -= first
    if need_v:
        img = ref._pass(img, (kv, bv, cv), 0)
    return img


# ---- the select rule ----------------------------------------------------------------------------------------------------------
def box_ok(b, w, h):
    x0, y0, x1, y1 = b
    return bool(np.isfinite(np.array(b, f32)).all() and 0 <= x0 < x1 <= w and 0 <= y0 < y1 <= h)


def pad_box(b, w, h, pad):
    """float32, one rounding per operation: bw = x1 - x0; x0' = max(x0 - pad * bw, 0); x1' = min(x1 + pad * bw, w)."""
    x0, y0, x1, y1 = (f32(v) for v in b)
    pad = f32(pad)
    bw, bh = f32(x1 - x0), f32(y1 - y0)
    return (max(f32(x0 - f32(pad * bw)), f32(0)), max(f32(y0 - f32(pad * bh)), f32(0)),
            min(f32(x1 + f32(pad * bw)), f32(w)), min(f32(y1 + f32(pad * bh)), f32(h)))


def select_rows(dets, count, sizes, thresh, pad, top_k=None):
    """dets float32 [n, K, 6] (class, score, x0, y0, x1, y1), count [n], sizes = [(h, w)] -> (src list of (image, row), boxes
    list of 4 float32), image-major and row-ascending.  A row is taken iff it lies in front of min(count, K), its six values are
    finite, class >= 0, score >= thresh, its own box and its padded box satisfy 0 <= x0 < x1 <= w and 0 <= y0 < y1 <= h, and
    fewer than top_k rows of its image were taken before it."""
    dets = np.asarray(dets, f32)
    n, K = dets.shape[:2]
    src, boxes = [], []
    with np.errstate(all='ignore'):
        for i in range(n):
            h, w = sizes[i]
            taken = 0
            for r in range(min(int(count[i]), K)):
                row = dets[i, r]
                if not np.isfinite(row).all() or not row[0] >= 0 or not row[1] >= f32(thresh):
                    continue
                if not box_ok(row[2:], w, h):
                    continue
                b = pad_box(row[2:], w, h, pad)
                if not box_ok(b, w, h):
                    continue
                if top_k is not None and taken >= top_k:
                    continue
                taken += 1
                src.append((i, r))
                boxes.append(b)
    return src, boxes


def select_list(boxes_in, image, sizes):
    """The list form: entry e is taken iff image[e] is an image of the batch and its box passes box_ok; list order."""
    src, boxes = [], []
    for e, (b, i) in enumerate(zip(np.asarray(boxes_in, f32), image)):
        if 0 <= i < len(sizes) and box_ok(b, sizes[i][1], sizes[i][0]):
            src.append((int(i), e))
            boxes.append(tuple(b))
    return src, boxes


# ---- the cases the tests and the golden share ----------------------------------------------------------------------------------
def seeded_cases(seed=26, count=24):
    """((h, w), (ow, oh), box): sources 1..90, outputs 1..40, boxes alternately fractional and integer, some touching the borders."""
    rng = np.random.RandomState(seed)
    cases = []
    for i in range(count):
        h, w = int(rng.randint(1, 91)), int(rng.randint(1, 91))
        ow, oh = int(rng.randint(1, 41)), int(rng.randint(1, 41))
        if i & 1:                                   # integer box
            x0 = int(rng.randint(0, w))
            x1 = int(rng.randint(x0 + 1, w + 1))
            y0 = int(rng.randint(0, h))
            y1 = int(rng.randint(y0 + 1, h + 1))
        else:                                       # fractional
            xs = np.sort(rng.uniform(0, w, 2))
            ys = np.sort(rng.uniform(0, h, 2))
            x0, x1, y0, y1 = float(xs[0]), float(xs[1]), float(ys[0]), float(ys[1])
            if i % 8 == 0:
                x0, y1 = 0.0, float(h)                # touching two borders
            if i % 8 == 4:
                x1, y0 = float(w), 0.0
        if f32(x1) - f32(x0) <= 0 or f32(y1) - f32(y0) <= 0:
            x0, y0, x1, y1 = 0.0, 0.0, float(w), float(h)
        cases.append(((h, w), (ow, oh), (x0, y0, x1, y1)))
    return cases


NAMED_CASES = [
    ((30, 20), (8, 6), (4, 3, 20, 15)),             # THE distinguishing case: differs from crop().resize()
    ((37, 53), (16, 16), (10.25, 7.5, 10.75, 30.0)),      # a box below one pixel: 0.5 px wide
    ((40, 33), (12, 9), (0, 5.5, 33, 31.25)),       # x0 = 0 with x1 = w
    ((25, 17), (17, 11), (0, 0, 17, 25)),           # the full-image box with ow == w: the horizontal pass is skipped
    ((25, 17), (9, 25), (0, 0, 17, 25)),            # ... with oh == h: the vertical pass is skipped
    ((25, 17), (17, 25), (0, 0, 17, 25)),           # ... both: a copy
    ((25, 17), (17, 11), (0, 2.5, 17, 20)),         # ow == w, x whole, y boxed: horizontal skipped, vertical boxed
    ((25, 17), (17, 25), (1, 0, 17, 25)),           # same size, the box is not the whole axis: the pass runs
]
CASES = NAMED_CASES + seeded_cases()
TAPS_CASE = ((16, 600), (4, 5), (0, 1.5, 600, 14.25))      # 16 x 600 source to ow = 4: LANCZOS reads 901 taps
DISTINGUISHING = NAMED_CASES[0]


def case_key(case):
    (h, w), (ow, oh), box = case
    return '%dx%d_%dx%d_%s' % (h, w, ow, oh, '_'.join('%g' % float(f32(v)) for v in box))


def case_image(case, kind):
    (h, w), (ow, oh), _ = case
    return ref.content(h, w, kind, ref.case_seed(h, w, ow, oh))


# hand-written rows for the select rule: three images of (h, w) = (40, 50), (33, 21), (64, 64); K = 8
SELECT_SIZES = [(40, 50), (33, 21), (64, 64)]
SELECT_THRESH = 0.5
NAN = float('nan')


def select_rows_case():
    g = [7.0, NAN, NAN, 1.0, NAN, 3.0]                     # garbage behind count
    d = np.array([
        [[3, 0.5, 10, 5, 30, 25],                          # score == thresh: taken
         [-1, 0.9, 10, 5, 30, 25],                         # class -1: skipped
         [2, 0.9, NAN, 5, 30, 25],                         # a NaN coordinate: skipped
         [2, 0.9, 12, 5, 12, 25],                          # x1 == x0: skipped
         [2, 0.9, 12, 5, 50.5, 25],                        # x1 > w: skipped
         [5, 0.8, 1.5, 12, 30, 39.5],                      # taken; pad = 0.1 clips it at two borders (x0 -> 0, y1 -> h)
         [1, 0.4, 10, 5, 30, 25],                          # below thresh: skipped
         g],                                               # count[0] = 7: never read
        [[0, 0.99, 0, 0, 21, 33],                          # the whole image: taken
         [0, 0.97, 2.5, 3.5, 8.25, 30],                    # taken
         g, g, g, g, g, g],                                # count[1] = 2
        [[4, 0.7, 3, 4, 60, 61]] * 8,                      # count[2] = 11 > K: all eight rows are read
    ], dtype=f32)
    count = np.array([7, 2, 11], np.int32)
    return d, count
