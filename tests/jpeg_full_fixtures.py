"""tests/golden/g22_jpeg_full.npz (tools/make_jpeg_full_goldens.py) as the tests of JpegDecoder(accept=...) read it."""
import hashlib
import os

import numpy as np

import jpeg_full_ref

_G = None


def golden():
    global _G
    if _G is None:
        _G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g22_jpeg_full.npz'))
    return _G


def names(large=True):
    return [str(n) for n in golden()['names'] if large or 'bgr_' + str(n) in golden()]


def incomplete():
    return [str(n) for n in golden()['incomplete']]


def data(name):
    return golden()['jpg_' + name].tobytes()


def matches_golden(name, px):
    """px == what libjpeg-turbo (Pillow) decoded when the fixture was made: pixels, or shape + SHA-256 for the large files."""
    g = golden()
    if 'bgr_' + name in g:
        return px.shape == g['bgr_' + name].shape and np.array_equal(px, g['bgr_' + name])
    return tuple(g['shape_' + name]) == px.shape and px.dtype == np.uint8 and \
        hashlib.sha256(np.ascontiguousarray(px).tobytes()).hexdigest() == str(g['sha_' + name])


_HD = {}


def coefficients(name):
    """The restatement's coefficient dict of a fixture, computed once; read-only."""
    if name not in _HD:
        _HD[name] = jpeg_full_ref.coefficients(data(name))
    return _HD[name]
