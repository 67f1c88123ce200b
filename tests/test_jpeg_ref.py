"""tests/jpeg_ref.py, the numpy restatement of the JPEG decoder, against libjpeg-turbo: the committed goldens (always) and
Pillow on freshly encoded seeded images (Pillow is built on libjpeg-turbo; the two tests that need it fail without it).  Array equality only."""
import io

import numpy as np
import pytest

import jpeg_fixtures as F
import jpeg_ref as R


def test_golden_covers_the_matrix():
    names = F.names()
    for want in ('c444', 'c422', 'c420', 'grey', 'dri', 'opt', 'q16', 'noise_q100', 'narrow', '1x1', 'segments', 'coco_'):
        assert any(want in n for n in names), want
    assert sum(n.startswith('orient') for n in names) == 8 and sum(n.startswith('coco_') for n in names) >= 2
    assert [k for _, k in F.refused()] == ['unsupported', 'corrupt']
    orients = sorted(R.parse(F.data(n))['orientation'] for n in names if n.startswith('orient'))
    assert orients == list(range(1, 9))


def test_golden_has_a_16_bit_table():
    def precisions(b):
        i, out = 2, []
        while b[i + 1] != 0xDA:
            L = b[i + 2] << 8 | b[i + 3]
            if b[i + 1] == 0xDB:
                out.append(b[i + 4] >> 4)
            i += 2 + L
        return out
    assert 1 in precisions(F.data('c420_q16_45x61'))


@pytest.mark.parametrize('name', F.names())
def test_ref_equals_golden(name):
    px = R.decode(F.data(name))
    assert px.dtype == np.uint8 and F.matches_golden(name, px)
    assert F.matches_golden(name, R.decode(F.data(name), apply_orientation=False), oriented=False)


@pytest.mark.parametrize('name,kind', F.refused())
def test_ref_refuses(name, kind):
    with pytest.raises(R.JpegUnsupported if kind == 'unsupported' else R.JpegCorrupt):
        R.decode(F.data(name))


def _smooth(rng, h, w):
    yy, xx = np.mgrid[:h, :w]
    a = np.stack([127 + 100 * np.sin(xx / 7. + k) * np.cos(yy / 5. - k) for k in range(3)], -1) + rng.normal(0, 12, (h, w, 3))
    return np.clip(a, 0, 255).astype(np.uint8)


SIZES = [(37, 53), (16, 16), (8, 24), (65, 33), (1, 1), (3, 2), (17, 1), (1, 19), (2, 3), (5, 4), (6, 5), (9, 6), (23, 7)]
MODES = [dict(subsampling=0), dict(subsampling=1), dict(subsampling=2), dict(subsampling=2, restart_marker_blocks=2),
         dict(subsampling=1, restart_marker_blocks=1, optimize=True), dict(subsampling=0, optimize=True, quality=35),
         dict(subsampling=2, quality=100), dict(grey=True), dict(grey=True, quality=50, restart_marker_blocks=3)]


def test_ref_equals_pillow_on_fresh_encodes():
    from PIL import Image, ImageOps          # a plain import: without Pillow this pin fails, it does not skip
    rng = np.random.default_rng(7)
    cases = 0
    for h, w in SIZES:
        for kw in MODES:
            kw = dict(kw)
            a = _smooth(rng, h, w)
            im = Image.fromarray(a[:, :, 0]) if kw.pop('grey', False) else Image.fromarray(a)
            kw.setdefault('quality', 90)
            bio = io.BytesIO()
            im.save(bio, 'JPEG', **kw)
            want = np.asarray(ImageOps.exif_transpose(Image.open(io.BytesIO(bio.getvalue()))).convert('RGB'))[:, :, ::-1]
            assert np.array_equal(R.decode(bio.getvalue()), want), ((h, w), kw)
            cases += 1
    # saturated noise at quality 100: the range-limit table wraps
    for sub in (0, 1, 2):
        a = (rng.random((40, 40, 3)) > 0.5).astype(np.uint8) * 255
        bio = io.BytesIO()
        Image.fromarray(a).save(bio, 'JPEG', quality=100, subsampling=sub)
        want = np.asarray(Image.open(io.BytesIO(bio.getvalue())).convert('RGB'))[:, :, ::-1]
        assert np.array_equal(R.decode(bio.getvalue()), want), sub
        cases += 1
    assert cases == len(SIZES) * len(MODES) + 3


def test_ref_orientation_equals_pillow():
    from PIL import Image, ImageOps          # a plain import: without Pillow this pin fails, it does not skip
    for name in F.names():
        if name.startswith('orient'):
            im = Image.open(io.BytesIO(F.data(name)))
            want = np.asarray(ImageOps.exif_transpose(im).convert('RGB'))[:, :, ::-1]
            assert np.array_equal(R.decode(F.data(name)), want), name
            assert np.array_equal(R.decode(F.data(name), apply_orientation=False), np.asarray(im.convert('RGB'))[:, :, ::-1])
