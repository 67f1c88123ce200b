"""tests/golden/g20_jpeg.npz (tools/make_jpeg_goldens.py) as the JPEG tests read it."""
import hashlib
import os

import numpy as np

import jpeg_ref

_G = None


def golden():
    global _G
    if _G is None:
        _G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g20_jpeg.npz'))
    return _G


def names():
    return [str(n) for n in golden()['names']]


def refused():
    """[(name, 'unsupported' | 'corrupt')]"""
    g = golden()
    return [(str(n), 'unsupported') for n in g['unsupported']] + [(str(n), 'corrupt') for n in g['corrupt']]


def data(name):
    return golden()['jpg_' + name].tobytes()


def matches_golden(name, px, oriented=True):
    """px == what libjpeg-turbo (Pillow) decoded when the fixture was made: pixels, or shape + SHA-256 for the large files."""
    g = golden()
    if not oriented and 'raw_' + name in g:
        return np.array_equal(px, g['raw_' + name])
    if 'bgr_' + name in g:
        return np.array_equal(px, g['bgr_' + name])
    return tuple(g['shape_' + name]) == px.shape and px.dtype == np.uint8 and \
        hashlib.sha256(np.ascontiguousarray(px).tobytes()).hexdigest() == str(g['sha_' + name])


_PIXELS = {}


def pixels(name, oriented=True):
    """The golden pixels; for the large files (stored as a hash) the restatement's output, checked against that hash."""
    key = (name, oriented)
    if key not in _PIXELS:
        px = jpeg_ref.decode(data(name), apply_orientation=oriented)
        assert matches_golden(name, px, oriented), name
        _PIXELS[key] = px
    return _PIXELS[key]
