#!/usr/bin/env python
"""Generate tests/golden/g21_jpeg_encode.npz: pixels with the JPEG files libjpeg-turbo writes from them.

Needs Pillow, which is built on libjpeg-turbo (features.check_feature('libjpeg_turbo')); the tests never need it.  The cases
are tests/jpeg_enc_cases.golden_subset(), a seeded subset of the grid tests/test_jpeg_enc_ref.py sweeps.  Per case NAME the
archive holds
    px_NAME     the pixels, uint8 [h,w,3] BGR or [h,w] grey
    jpg_NAME    Image.fromarray(rgb).save(buf, 'JPEG', quality=q, subsampling=s[, restart_marker_blocks=r]), uint8
and `cases`: one row (name, subsampling, quality, restart interval) per case, as strings.  The two COCO-sized fixtures of
tests/golden/g20_jpeg.npz are encoded from their decoded pixels (jpeg_fixtures.pixels) and stored by name as len_NAME and
sha_NAME (SHA-256 of the file) only: their pixels are taken from g20 at test time.

    python tools/make_jpeg_encode_goldens.py
"""
import hashlib
import io
import os
import sys

import numpy as np
from PIL import Image, features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'g21_jpeg_encode.npz')
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import jpeg_enc_cases as C  # noqa: E402
import jpeg_fixtures as F  # noqa: E402


def pillow(img, subsampling, quality, restart):
    kw = dict(quality=quality)
    if img.ndim == 3:
        kw['subsampling'] = subsampling
    if restart:
        kw['restart_marker_blocks'] = restart
    bio = io.BytesIO()
    Image.fromarray(img if img.ndim == 2 else np.ascontiguousarray(img[:, :, ::-1])).save(bio, 'JPEG', **kw)
    return bio.getvalue()


def main():
    assert features.check_feature('libjpeg_turbo'), 'this Pillow is not built on libjpeg-turbo'
    out, cases = {}, []
    for name, content, w, h, s, q, r in C.golden_subset():
        img = C.image(content, w, h, s == 'grey')
        out['px_' + name] = img
        out['jpg_' + name] = np.frombuffer(pillow(img, s, q, r), np.uint8)
        cases.append((name, s, str(q), str(r)))
    for name, s, q, r in C.COCO:
        b = pillow(F.pixels(name), s, q, r)
        out['len_' + name] = np.int64(len(b))
        out['sha_' + name] = np.array(hashlib.sha256(b).hexdigest())
    out['cases'] = np.array(cases)
    np.savez_compressed(OUT, **out)
    print('%s: %d cases, %d bytes' % (OUT, len(cases), os.path.getsize(OUT)))


if __name__ == '__main__':
    main()
