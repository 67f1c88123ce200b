#!/usr/bin/env python
"""Generate tests/golden/g20_jpeg.npz: encoded JPEG byte strings with the pixels libjpeg-turbo decodes from them.

Needs Pillow, which is built on libjpeg-turbo, and a checkout of the reference (miemie2013/Pytorch-PPYOLO): the two
smallest files of its images/test/ are the COCO-sized fixtures.  Runs where both are; the tests never need either.
Per fixture NAME the archive holds
    jpg_NAME    the file, uint8
    bgr_NAME    Pillow's pixels as cv2.imread orders them (BGR, EXIF orientation applied), uint8 [h,w,3]; or, for the large
                files, sha_NAME = SHA-256 of those bytes and shape_NAME
    raw_NAME    the same without the orientation step, only where the orientation is not 1
and `names`, `unsupported` (files the decoder must refuse as outside its subset) and `corrupt` (damaged files).

    python tools/make_jpeg_goldens.py REFERENCE_DIR
"""
import glob
import hashlib
import io
import os
import struct
import sys

import numpy as np
from PIL import Image, ImageOps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'g20_jpeg.npz')


def smooth(rng, h, w):
    yy, xx = np.mgrid[:h, :w]
    a = np.stack([127 + 100 * np.sin(xx / 7. + k) * np.cos(yy / 5. - k) for k in range(3)], -1) + rng.normal(0, 12, (h, w, 3))
    return np.clip(a, 0, 255).astype(np.uint8)


def encode(a, **kw):
    bio = io.BytesIO()
    kw.setdefault('quality', 90)
    Image.fromarray(a).save(bio, 'JPEG', **kw)
    return bio.getvalue()


def exif_segment(orientation, big_endian=False):
    e = '>' if big_endian else '<'
    tiff = (b'MM' if big_endian else b'II') + struct.pack(e + 'HI', 42, 8) + struct.pack(e + 'H', 1) + \
        struct.pack(e + 'HHIHH', 0x0112, 3, 1, orientation, 0) + struct.pack(e + 'I', 0)
    body = b'Exif\0\0' + tiff
    return b'\xff\xe1' + struct.pack('>H', len(body) + 2) + body


def insert_after_soi(b, extra):
    assert b[:2] == b'\xff\xd8'
    return b[:2] + extra + b[2:]


def widen_dqt(b):
    """Rewrite every 8-bit quantisation table of the file as a 16-bit one (Pq = 1) with the same values."""
    out, i = bytearray(b[:2]), 2
    while True:
        m, L = b[i + 1], struct.unpack('>H', b[i + 2:i + 4])[0]
        s = b[i + 4:i + 2 + L]
        if m == 0xDB:
            body, j = bytearray(), 0
            while j < len(s):
                assert s[j] >> 4 == 0
                body.append(0x10 | s[j])
                body += b''.join(struct.pack('>H', v) for v in s[j + 1:j + 65])
                j += 65
            out += b'\xff\xdb' + struct.pack('>H', len(body) + 2) + body
        else:
            out += b[i:i + 2 + L]
        i += 2 + L
        if m == 0xDA:
            return bytes(out + b[i:])


def pillow_bgr(b, oriented=True):
    im = Image.open(io.BytesIO(b))
    if oriented:
        im = ImageOps.exif_transpose(im)
    return np.ascontiguousarray(np.asarray(im.convert('RGB'))[:, :, ::-1])


def main():
    ref_images = os.path.join(sys.argv[1], 'images', 'test')
    rng = np.random.default_rng(20)
    fx = {}
    fx['c444_37x53'] = encode(smooth(rng, 37, 53), subsampling=0)
    fx['c422_37x53'] = encode(smooth(rng, 37, 53), subsampling=1)
    fx['c420_37x53'] = encode(smooth(rng, 37, 53), subsampling=2)
    fx['grey_29x43'] = encode(smooth(rng, 29, 43)[:, :, 0])
    fx['c420_dri_65x33'] = encode(smooth(rng, 65, 33), subsampling=2, restart_marker_blocks=2)
    fx['c422_dri_opt_41x70'] = encode(smooth(rng, 41, 70), subsampling=1, restart_marker_blocks=3, optimize=True, quality=60)
    fx['c444_opt_q35_50x50'] = encode(smooth(rng, 50, 50), subsampling=0, optimize=True, quality=35)
    fx['c420_q16_45x61'] = widen_dqt(encode(smooth(rng, 45, 61), subsampling=2, quality=75))
    try:        # a table that NEEDS 16 bits, if this Pillow emits one
        big = encode(smooth(rng, 20, 27), subsampling=0, qtables=[[min(16 + 9 * k, 600) for k in range(64)]] * 2)
        if b'\xff\xdb' in big and pillow_bgr(big).shape == (20, 27, 3):
            fx['c444_q16big_20x27'] = big
    except Exception as e:          # noqa: BLE001 -- any refusal means "cannot emit"
        print('Pillow does not emit 16-bit tables:', e)
    fx['noise_q100_40x40'] = encode((rng.random((40, 40, 3)) > 0.5).astype(np.uint8) * 255, quality=100, subsampling=2)
    fx['c420_narrow_19x3'] = encode(smooth(rng, 19, 3), subsampling=2)           # chroma 2 columns wide
    fx['c422_narrow_9x4'] = encode(smooth(rng, 9, 4), subsampling=1)
    fx['c420_narrow_17x1'] = encode(smooth(rng, 17, 1), subsampling=2)
    fx['c420_1x1'] = encode(smooth(rng, 1, 1), subsampling=2)
    fx['c420_5x5'] = encode(smooth(rng, 5, 5), subsampling=2)                   # chroma 3 columns: the narrowest fancy case
    base = encode(smooth(rng, 21, 13), subsampling=2)
    for o in range(1, 9):
        fx['orient%d_21x13' % o] = insert_after_soi(base, exif_segment(o, big_endian=o % 2 == 0))
    junk = b'\xff\xe2' + struct.pack('>H', 2 + 40) + bytes(range(40)) + b'\xff\xfe' + struct.pack('>H', 2 + 11) + b'hello world' + \
        b'\xff\xff\xff\xed' + struct.pack('>H', 2 + 7) + b'\xff\xd8\xff\xc2\x00\xff\xda'
    fx['segments_33x35'] = insert_after_soi(encode(smooth(rng, 33, 35), subsampling=2), junk)
    files = sorted(glob.glob(os.path.join(ref_images, '*.jpg')), key=os.path.getsize)[:2]
    for f in files:
        fx['coco_' + os.path.basename(f)[:-4].lstrip('0')] = open(f, 'rb').read()
    unsupported = {'progressive_30x30': encode(smooth(rng, 30, 30), progressive=True)}
    full = fx['c420_37x53']
    corrupt = {'truncated_c420_37x53': full[:len(full) * 6 // 10]}

    out = dict(names=np.array(sorted(fx)), unsupported=np.array(sorted(unsupported)), corrupt=np.array(sorted(corrupt)))
    for name, b in list(fx.items()) + list(unsupported.items()) + list(corrupt.items()):
        out['jpg_' + name] = np.frombuffer(b, np.uint8)
    for name, b in fx.items():
        px = pillow_bgr(b)
        if px.size > 1 << 16:
            out['sha_' + name] = np.array(hashlib.sha256(px.tobytes()).hexdigest())
            out['shape_' + name] = np.array(px.shape)
        else:
            out['bgr_' + name] = px
        raw = pillow_bgr(b, oriented=False)
        if raw.shape != px.shape or not np.array_equal(raw, px):
            out['raw_' + name] = raw
    np.savez_compressed(OUT, **out)
    print('%s: %d fixtures, %.1f KB' % (OUT, len(fx) + 2, os.path.getsize(OUT) / 1024.0))
    for name in sorted(fx):
        print('  %-24s %6d bytes' % (name, len(fx[name])))


if __name__ == '__main__':
    main()
