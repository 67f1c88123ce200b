"""tests/jpeg_enc_ref.py == libjpeg-turbo, byte for byte: the numpy restatement of the encoder against Pillow's
Image.save(buf, 'JPEG', quality=q, subsampling=s[, restart_marker_blocks=r]) over the whole seeded grid of
tests/jpeg_enc_cases.py, and against the stored goldens.  The grid must reach every path of the entropy coder and of the
block grid by the restatement's own flags, so an input choice cannot quietly miss one."""
import io

import numpy as np
import PIL
from PIL import Image, features

import jpeg_enc_cases as C
import jpeg_enc_ref as E
import jpeg_fixtures as F
import jpeg_ref as R


def pillow(img, subsampling, quality, restart):
    kw = dict(quality=quality)
    if img.ndim == 3:
        kw['subsampling'] = subsampling
    if restart:
        kw['restart_marker_blocks'] = restart
    bio = io.BytesIO()
    Image.fromarray(img if img.ndim == 2 else np.ascontiguousarray(img[:, :, ::-1])).save(bio, 'JPEG', **kw)
    return bio.getvalue()


def test_pillow_is_libjpeg_turbo():
    assert PIL.__version__ and features.check_feature('libjpeg_turbo')


def test_restatement_equals_pillow_over_the_grid():
    flags, wrong, n = set(), [], 0
    for name, content, w, h, s, q, r in C.grid():
        img = C.image(content, w, h, s == 'grey')
        got, hd, fl = E.encode(img, q, s if s != 'grey' else '4:4:4', r)
        flags |= fl
        n += 1
        if got != pillow(img, s, q, r):
            wrong.append(name)
    assert n == 3 * 10 * 4 * 8 * 3 + 10 * 4 * 3
    assert not wrong, wrong[:10]
    assert flags == set(E.FLAGS), 'the grid misses %s' % sorted(set(E.FLAGS) - flags)


def test_segment_order_and_app0():
    """SOI, APP0(16), DQT(67), DQT(67), SOF0(17), DHT(31), DHT(181), DHT(31), DHT(181), [DRI(4)], SOS; a grey file has one DQT
    and two DHTs; the APP0 payload is JFIF 1.01, units 0, density 1:1, no thumbnail."""
    def segments(b):
        out, i = [], 2
        while True:
            m, ln = b[i + 1], int.from_bytes(b[i + 2:i + 4], 'big')
            out.append((m, ln))
            i += 2 + ln
            if m == 0xDA:
                return out
    img = C.image('smooth', 16, 16, False)
    for r in (0, 3):
        b = pillow(img, '4:2:0', 75, r)
        assert b == E.encode(img, 75, '4:2:0', r)[0]
        want = [(0xE0, 16), (0xDB, 67), (0xDB, 67), (0xC0, 17), (0xC4, 31), (0xC4, 181), (0xC4, 31), (0xC4, 181)] + [(0xDD, 4)] * bool(r) + [(0xDA, 12)]
        assert segments(b) == want
        assert b[6:20].hex() == '4a464946000101000001' + '00010000'
    g = C.image('smooth', 16, 16, True)
    assert segments(pillow(g, None, 75, 0)) == [(0xE0, 16), (0xDB, 67), (0xC0, 11), (0xC4, 31), (0xC4, 181), (0xDA, 8)]


def test_dummy_blocks_copy_the_dc_before_them():
    """An 8x8 image at 4:2:0 and quality 100 with a vertical edge: four luma blocks with DC -104 each, only the first has AC."""
    img = np.zeros((8, 8, 3), np.uint8)
    img[:, 6:] = 255
    data, hd, fl = E.encode(img, 100, '4:2:0', 0)
    assert data == pillow(img, '4:2:0', 100, 0)
    back = R.coefficients(data)['comps'][0]['coef'].reshape(4, 64)
    assert (back[:, 0] == back[0, 0]).all() and back[0, 1:].any() and not back[1:, 1:].any()
    assert np.array_equal(back, hd['comps'][0]['coef'].reshape(4, 64))
    assert fl >= {'dummy_right', 'dummy_below', 'dummy_both'}


def test_padding_rules():
    """The two rules Pillow settled: right of the image the full-resolution PIXELS replicate and the box
    filter runs over them; below it the last row of SAMPLES replicates.  An 8x8 image at 4:2:0 with distinct last columns and
    rows tells both from their alternatives."""
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (8, 8, 3), dtype=np.uint8)
    for s in ('4:2:0', '4:2:2'):
        assert E.encode(img, 100, s, 0)[0] == pillow(img, s, 100, 0)
    cb = E.ycc(img)[1]
    plane = E.component_plane(cb, 2, 2, 1, 1)
    assert np.array_equal(plane[4:], np.repeat(plane[3:4], 4, 0))                       # sample rows repeat
    assert np.array_equal(plane[:4, 4], (2 * cb[0::2, 7] + 2 * cb[1::2, 7] + 1) >> 2)     # pixels repeat, then the filter (bias 1 at column 4)


def test_goldens_are_what_pillow_writes_and_the_restatement_too():
    for name, s, q, r in C.golden_cases():
        img = C.golden_pixels(name)
        want = C.golden_bytes(name)
        assert pillow(img, s, q, r) == want, name
        assert E.encode(img, q, s if s != 'grey' else '4:4:4', r)[0] == want, name
    for name, s, q, r in C.COCO:
        px = F.pixels(name)
        assert C.matches_coco(name, pillow(px, s, q, r)), name
        assert C.matches_coco(name, E.encode(px, q, s, r)[0]), name


def test_quantiser_tables():
    for q in C.QUALITIES:
        hd = R.parse(pillow(C.image('flat', 8, 8, False), '4:4:4', q, 0))
        lum, chrom = E.quant_tables(q)
        assert np.array_equal(hd['q'][0], lum) and np.array_equal(hd['q'][1], chrom)
