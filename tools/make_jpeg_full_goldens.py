#!/usr/bin/env python
"""Generate tests/golden/g22_jpeg_full.npz: the files JpegDecoder(accept='all') adds to the baseline subset, each with the
pixels libjpeg-turbo decodes from it.

Needs Pillow (built on libjpeg-turbo); the tests that read the archive do not.  Two families:
    pil_*   written by Pillow: progressive, quality 35 / 75 / 95, subsampling 0 / 1 / 2 and grey, with and without restart
            markers, one with EXIF orientation 6, at 1x1, 7x9, 17x23, 37x53 and 300 wide; and the two COCO-sized fixtures of
            g20_jpeg.npz re-encoded as progressive files (their pixels as SHA-256 + shape);
    syn_*   written from seeded coefficients by tests/jpeg_full_synth.py, which Pillow cannot write: the further luma
            factors (4:4:0, 4:1:1, 4:1:0, 1x4, 3x1, ...) at 1x1, 3x2, 5x9, 17x23 and 40x70 as single-scan, multi-scan and
            progressive files, and multi-scan sequential files of the baseline samplings.
Per fixture NAME: jpg_NAME (the file), bgr_NAME (Pillow's pixels, BGR, orientation applied) or sha_NAME + shape_NAME; and
`names`, `incomplete` (progressive files with a deliberately incomplete scan script: no pixels) and `pillow` (the version
that decoded them).  17 wide / high at 4:2:0 has 3 real luma block columns / rows against 4 padded ones; 5 wide at 4:1:1
and 2 high at 4:4:0 give a chroma plane 2 wide / 1 high.

    python tools/make_jpeg_full_goldens.py
"""
import hashlib
import io
import os
import sys

import numpy as np
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import jpeg_full_synth as FS          # noqa: E402
import jpeg_synth as S                # noqa: E402
from make_jpeg_goldens import exif_segment, insert_after_soi, pillow_bgr, smooth          # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'g22_jpeg_full.npz')
PIL_SIZES = [(1, 1), (9, 7), (23, 17), (53, 37), (40, 300)]                 # (H, W)
SYN_SIZES = [(1, 1), (2, 3), (9, 5), (23, 17), (70, 40)]


def encode(a, **kw):
    bio = io.BytesIO()
    Image.fromarray(a).save(bio, 'JPEG', progressive=True, **kw)
    return bio.getvalue()


def main():
    rng = np.random.default_rng(22)
    fx, incomplete = {}, {}
    k = 0
    for H, W in PIL_SIZES:
        for sub in (0, 1, 2, 'grey'):
            q = (35, 75, 95)[k % 3]
            dri = (0, 1, 3, 0)[(k // 3 + k) % 4]
            a = smooth(rng, H, W)
            kw = dict(quality=q)
            if dri:
                kw['restart_marker_blocks'] = dri
            if sub == 'grey':
                a = a[:, :, 0]
            else:
                kw['subsampling'] = sub
            name = 'pil_%s_q%d%s_%dx%d' % ({0: 'p444', 1: 'p422', 2: 'p420', 'grey': 'pgrey'}[sub], q, '_dri%d' % dri if dri else '', W, H)
            fx[name] = encode(a, **kw)
            k += 1
    fx['pil_p420_q75_orient6_17x23'] = insert_after_soi(encode(smooth(rng, 23, 17), quality=75, subsampling=2), exif_segment(6))
    g20 = np.load(os.path.join(ROOT, 'tests', 'golden', 'g20_jpeg.npz'))
    for n in [str(n) for n in g20['names'] if str(n).startswith('coco_')]:
        rgb = np.asarray(Image.open(io.BytesIO(g20['jpg_' + n].tobytes())).convert('RGB'))
        fx['pil_p420_q75_' + n] = encode(rgb, quality=75, subsampling=2)

    kinds = ['single', 'scans3', 'scans12', 'default', 'spectral', 'deep']
    k = 0
    for lname, luma in FS.NEW_LUMA.items():
        for H, W in SYN_SIZES:
            kind = kinds[k % len(kinds)]
            dri = (0, 1, 3)[(k // 6 + k) % 3]
            tables = ('flat', 'skewed')[k // 6 % 2]
            hd = FS.synth(rng, H, W, luma, orientation=(1, 1, 6, 3, 8)[k % 5])
            fx['syn_%s_%s%s_%dx%d' % (lname, kind, '_dri%d' % dri if dri else '', W, H)] = write(hd, kind, dri, tables)
            k += 1
    for lname, luma in (('444', (1, 1)), ('422', (2, 1)), ('420', (2, 2))):       # multi-scan files of the baseline samplings
        for kind, (H, W) in (('scans3', (23, 17)), ('scans12', (17, 23))):
            fx['syn_%s_%s_dri2_%dx%d' % (lname, kind, W, H)] = write(FS.synth(rng, H, W, luma), kind, 2, 'skewed')
    for luma, lname in (((2, 2), '420'), ('grey', 'grey')):
        hd = FS.clear_padding(FS.synth(rng, 23, 17, luma))
        incomplete['syn_%s_incomplete_17x23' % lname] = FS.progressive(hd, FS.script_incomplete(len(hd['comps'])))

    out = dict(names=np.array(sorted(fx)), incomplete=np.array(sorted(incomplete)), pillow=np.array(PIL.__version__))
    for name, b in list(fx.items()) + list(incomplete.items()):
        out['jpg_' + name] = np.frombuffer(b, np.uint8)
    for name, b in fx.items():
        px = pillow_bgr(b)
        if px.size > 1 << 16:
            out['sha_' + name] = np.array(hashlib.sha256(px.tobytes()).hexdigest())
            out['shape_' + name] = np.array(px.shape)
        else:
            out['bgr_' + name] = px
    np.savez_compressed(OUT, **out)
    print('%s: %d fixtures, %.1f KB, Pillow %s' % (OUT, len(fx) + len(incomplete), os.path.getsize(OUT) / 1024.0, PIL.__version__))


def write(hd, kind, dri, tables):
    n = len(hd['comps'])
    if kind == 'single':
        return S.encode(hd, dri=dri, tables=tables)
    hd = FS.clear_padding(hd)
    if kind == 'scans3':
        return FS.sequential(hd, [[c] for c in range(n)], dri=dri, tables=tables)
    if kind == 'scans12':
        return FS.sequential(hd, [[0], [1, 2]], dri=dri, tables=tables)
    return FS.progressive(hd, FS.SCRIPTS[kind](n), dri=dri, tables=tables)


if __name__ == '__main__':
    main()
