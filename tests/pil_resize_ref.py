"""Pillow's `Image.resize((ow, oh), filter)` for 3-channel uint8 images, restated in numpy: the coefficient tables of one axis
and the pixels.  Every float is a Python float (an IEEE double, one rounding per operation, in Pillow's
order) and sin / cos are `math`'s, the C library's, as in Pillow's Resample.c -- numpy's vectorised sin may round differently.

tests/test_pil_resize_host.py pins this file to the installed Pillow and to tests/golden/g25_pil_resize.npz, and the
library's planner (csrc/pil_resize.hip) to this file, integer for integer."""
import functools
import math

import numpy as np

NEAREST, LANCZOS, BILINEAR, BICUBIC, BOX, HAMMING = range(6)      # Pillow's codes (PIL.Image.Resampling)
FILTERS = (NEAREST, LANCZOS, BILINEAR, BICUBIC, BOX, HAMMING)
NAMES = {NEAREST: 'nearest', LANCZOS: 'lanczos', BILINEAR: 'bilinear', BICUBIC: 'bicubic', BOX: 'box', HAMMING: 'hamming'}
SUPPORT = {BOX: 0.5, BILINEAR: 1.0, HAMMING: 1.0, BICUBIC: 2.0, LANCZOS: 3.0}
PRECISION_BITS = 22
F054, F046 = float(np.float32(0.54)), float(np.float32(0.46))      # Resample.c writes these two as float literals


def _box(x):
    return 1.0 if -0.5 < x <= 0.5 else 0.0


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _hamming(x):
    x = abs(x)
    if x == 0.0:
        return 1.0
    if x >= 1.0:
        return 0.0
    x = x * math.pi
    return math.sin(x) / x * (F054 + F046 * math.cos(x))


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


_FUNCS = {BOX: _box, BILINEAR: _bilinear, HAMMING: _hamming, BICUBIC: _bicubic, LANCZOS: _lanczos}


def ksize_of(insz, outsz, f):
    return int(math.ceil(SUPPORT[f] * max(insz / outsz, 1.0))) * 2 + 1


@functools.lru_cache(None)
def axis_table(insz, outsz, f):
    """Filters 1..5, one axis: (ksize, bounds int32 [out, 2] = (xmin, count), k int32 [out, ksize], zero past count).  Cached: the
    arrays are shared, do not write to them."""
    fn = _FUNCS[f]
    scale = insz / outsz
    fs = max(scale, 1.0)
    support = SUPPORT[f] * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    bounds = np.zeros((outsz, 2), np.int32)
    k = np.zeros((outsz, ksize), np.int32)
    for xx in range(outsz):
        center = (xx + 0.5) * scale
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
            k[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
    return ksize, bounds, k


def nearest_map(insz, outsz):
    """NEAREST, one axis: int32 [out] source indices; the coordinate is accumulated by repeated addition, as Pillow's affine
    scaler does."""
    step = insz / outsz
    xo = step * 0.5
    idx = np.zeros(outsz, np.int32)
    for x in range(outsz):
        idx[x] = int(math.floor(xo))
        xo += step
    return idx


def _pass(img, table, axis):
    """One separable pass over `axis` (0 rows, 1 columns) of a uint8 [h, w, 3] image."""
    ksize, bounds, k = table
    img = np.moveaxis(img, axis, 0)
    out = np.empty((bounds.shape[0],) + img.shape[1:], np.uint8)
    for xx in range(bounds.shape[0]):
        x0, cnt = int(bounds[xx, 0]), int(bounds[xx, 1])
        acc = np.tensordot(k[xx, :cnt].astype(np.int64), img[x0:x0 + cnt].astype(np.int64), axes=(0, 0)) + (1 << (PRECISION_BITS - 1))
        assert np.abs(acc).max() < 2 ** 31
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.ascontiguousarray(np.moveaxis(out, 0, axis))


def resize(img, ow, oh, f):
    """uint8 [h, w, 3] -> uint8 [oh, ow, 3], as Image.fromarray(img).resize((ow, oh), f)."""
    img = np.ascontiguousarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
    h, w = img.shape[:2]
    if (h, w) == (oh, ow):
        return img.copy()
    if f == NEAREST:
        return np.ascontiguousarray(img[nearest_map(h, oh)][:, nearest_map(w, ow)])
    if w != ow:
        img = _pass(img, axis_table(w, ow, f), 1)
    if h != oh:
        img = _pass(img, axis_table(h, oh, f), 0)
    return img


# ---- the cases the tests and the golden share ------------------------------------------------------------------------------
SMALL_CASES = [((37, 53), (16, 16)), ((13, 9), (32, 32)), ((16, 40), (16, 16)), ((40, 16), (16, 16)), ((16, 16), (16, 16)),
               ((1, 7), (8, 8)), ((200, 3), (32, 32)), ((64, 48), (20, 64))]      # ((h, w), (ow, oh))
LONG_CASE = ((1080, 1920), (64, 64))
COCO_CASE = ((480, 640), (608, 608))      # BICUBIC and LANCZOS only


def content(h, w, kind, seed):
    """Seeded uint8 [h, w, 3]: 'random' grey levels, or 'binary' 0 / 255 (drives the negative lobes into both clamps)."""
    rng = np.random.RandomState(seed)
    if kind == 'binary':
        return (rng.randint(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    return rng.randint(0, 256, (h, w, 3)).astype(np.uint8)


def case_seed(h, w, ow, oh):
    return (h * 7919 + w * 104729 + ow * 31 + oh) % (2 ** 31 - 1)
