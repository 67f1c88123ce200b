"""The synthesised PNG files the PNG tests share (tests/png_synth.py writes them, seeded): name -> bytes, made once per
process, and the expected pixels from the numpy restatement (tests/png_ref.py), computed once and handed out read-only.

GREY16 names the one case where Pillow departs from the contract: 16-bit grey without alpha opens
as mode I;16 and convert('RGB') clips to 255 instead of taking the high byte."""
import functools
import os
import zlib

import numpy as np

import png_ref
import png_synth as S

FORMATS = [(0, 1), (0, 2), (0, 4), (0, 8), (0, 16), (2, 8), (2, 16), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8), (4, 16), (6, 8), (6, 16)]
CYCLE = [0, 1, 2, 3, 4]
ADAM7_SIZES = [(1, 1), (2, 3), (4, 4), (5, 5), (8, 8), (9, 9), (23, 37)]      # (h, w): 3x2 and 37x23 are w x h
TILE = 16                                                                     # PNG_TILE of csrc/png.hip: units per LDS tile


def is_grey16(data):
    return data[24] == 16 and data[25] == 0


def _palette(rng, entries):
    return bytes(rng.randint(0, 256, 3 * entries).astype(np.uint8))


def _file(rng, h, w, ctype, depth, filters=CYCLE, interlace=0, two_valued=False, entries=None, **kw):
    entries = entries or (1 << depth)
    s = S.random_samples(rng, h, w, ctype, depth, two_valued, entries if ctype == 3 else None)
    return S.make_png(s, ctype, depth, filters, interlace, palette=_palette(rng, entries) if ctype == 3 else None, **kw)


@functools.lru_cache(None)
def edges():
    """1x1, 1xN, Nx1, a width that leaves no left neighbour; the first row under Up / Avg / Paeth, the first pixel under Sub /
    Avg / Paeth; the five filters cycling, a None or Sub row right after a Paeth row; two-valued content (Avg with a + b >=
    256, wrap-around sums); crafted Paeth ties."""
    rng = np.random.RandomState(2601)
    out = {}
    for ctype, depth in ((2, 8), (6, 16), (0, 8)):
        for h, w in ((1, 1), (1, 9), (9, 1), (2, 2), (5, 7)):
            for first in (0, 1, 2, 3, 4):
                out['edge_c%d_d%d_%dx%d_first%d' % (ctype, depth, h, w, first)] = _file(
                    rng, h, w, ctype, depth, filters=[first, 4, 0, 4, 1, 3, 2])
            out['edge_two_c%d_d%d_%dx%d' % (ctype, depth, h, w)] = _file(rng, h, w, ctype, depth, filters=[3, 4, 1, 2], two_valued=True)
    for ft in (1, 2, 3, 4):
        out['edge_two_all%d' % ft] = _file(rng, 9, 11, 2, 8, filters=ft, two_valued=True)
        out['edge_near_all%d' % ft] = S.make_png(rng.choice([0, 1, 2, 3, 253, 254, 255], size=(9, 11, 3)), 2, 8, ft)
    # Paeth ties, grey 8: the second row is Paeth; a = left, b = above, c = above-left of its second pixel
    for name, (c, b, a) in dict(abc_equal=(7, 7, 7), pa_eq_pb=(0, 10, 10), pb_eq_pc=(10, 8, 11), pa_eq_pc=(10, 11, 12),
                                all_eq_nonzero=(10, 12, 8), wrap=(255, 0, 255)).items():
        out['edge_tie_' + name] = S.make_png(np.array([[[c], [b]], [[a], [200]]]), 0, 8, [0, 4])
        out['edge_tie3_' + name] = S.make_png(np.array([[[c] * 3, [b] * 3], [[a] * 3, [200, 3, 77]]]), 2, 8, [1, 4])
    return out


@functools.lru_cache(None)
def formats():
    """Every colour type x depth pair; sub-byte depths at widths 1..9 and 15..17; palettes of 1, 16 and 256 entries, and one
    whose indices run past PLTE."""
    rng = np.random.RandomState(2602)
    out = {}
    for ctype, depth in FORMATS:
        out['fmt_c%d_d%d' % (ctype, depth)] = _file(rng, 5, 7, ctype, depth)
        out['fmt_two_c%d_d%d' % (ctype, depth)] = _file(rng, 6, 19, ctype, depth, two_valued=True)
    for ctype in (0, 3):
        for depth in (1, 2, 4):
            for w in list(range(1, 10)) + [15, 16, 17]:
                out['sub_c%d_d%d_w%d' % (ctype, depth, w)] = _file(rng, 3, w, ctype, depth)
    out['pal_1'] = _file(rng, 4, 9, 3, 1, entries=1)
    out['pal_16'] = _file(rng, 4, 9, 3, 4, entries=16)
    out['pal_16_of_8bit'] = _file(rng, 4, 9, 3, 8, entries=16)
    out['pal_256'] = _file(rng, 16, 16, 3, 8, entries=256)
    out['pal_short'] = S.make_png(rng.randint(0, 256, (4, 9, 1)), 3, 8, CYCLE, palette=_palette(rng, 5))      # indices past PLTE: black
    trns = S.chunk(b'tRNS', bytes([0, 128, 255]))
    out['trns_palette'] = S.make_png(rng.randint(0, 16, (5, 6, 1)), 3, 4, CYCLE, palette=_palette(rng, 16), before_idat=[trns])
    out['trns_grey'] = S.make_png(rng.randint(0, 256, (5, 6, 1)), 0, 8, CYCLE, before_idat=[S.chunk(b'tRNS', b'\x00\x07')])
    out['trns_rgb'] = S.make_png(rng.randint(0, 256, (5, 6, 3)), 2, 8, CYCLE, before_idat=[S.chunk(b'tRNS', b'\x00\x07\x00\x08\x00\x09')])
    return out


@functools.lru_cache(None)
def rows_and_widths():
    """Heights around the wave (63, 64, 65, 129), 1025 rows of 3 pixels and a wider image over the band hand-over; widths around
    the wave and just past the LDS staging tile."""
    rng = np.random.RandomState(2603)
    out = {}
    for h in (63, 64, 65, 129):
        out['rows_%d' % h] = _file(rng, h, 5, 2, 8)
    out['rows_1025x3'] = _file(rng, 1025, 3, 2, 8)
    out['rows_1030x40_rgba'] = _file(rng, 1030, 40, 6, 8)
    out['rows_1026x35_grey2_adam7'] = _file(rng, 2051, 35, 0, 2, interlace=1)      # passes of 1026 rows: a band hand-over per pass
    for w in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 63, 64, 65):
        out['width_%d' % w] = _file(rng, 4, w, 2, 8)
        out['width_%d_grey' % w] = _file(rng, 4, w, 0, 8)
    out['width_8x17_rgba16'] = _file(rng, 6, 8 * TILE + 1, 6, 16)
    return out


@functools.lru_cache(None)
def adam7():
    rng = np.random.RandomState(2604)
    out = {}
    for h, w in ADAM7_SIZES:
        for ctype, depth in ((0, 1), (2, 8), (6, 16)):
            out['adam7_c%d_d%d_%dx%d' % (ctype, depth, w, h)] = _file(rng, h, w, ctype, depth, interlace=1)
    return out


def all_cases():
    out = {}
    for part in (edges(), formats(), rows_and_widths(), adam7()):
        out.update(part)
    return out


_WANT = {}


def want(name):
    """The restatement's pixels of a case, computed once; read-only."""
    if name not in _WANT:
        px = png_ref.decode(all_cases()[name])
        px.setflags(write=False)
        _WANT[name] = px
    return _WANT[name]


# ---- tests/golden/g26_png.npz: a handful of the files above with the pixels the contract gives them ----------------------------
GOLDEN = ['fmt_c2_d8', 'fmt_c6_d16', 'fmt_c0_d16', 'fmt_c4_d16', 'sub_c0_d1_w9', 'sub_c3_d2_w17', 'pal_short', 'trns_palette',
          'adam7_c2_d8_37x23', 'adam7_c0_d1_9x9', 'adam7_c6_d16_3x2', 'edge_tie_pb_eq_pc', 'rows_65', 'width_17']
_G = None


def golden():
    global _G
    if _G is None:
        _G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g26_png.npz'))
    return _G


def write_golden(path):
    """Pixels: Pillow's where Pillow is the pin (asserted equal to the restatement), the restatement's for GREY16."""
    import io
    from PIL import Image
    cases = all_cases()
    arrays = dict(names=np.array(GOLDEN))
    for n in GOLDEN:
        px = want(n)
        if not is_grey16(cases[n]):
            assert np.array_equal(px, np.asarray(Image.open(io.BytesIO(cases[n])).convert('RGB'))[..., ::-1]), n
        arrays['png_' + n] = np.frombuffer(cases[n], np.uint8)
        arrays['bgr_' + n] = px
    np.savez_compressed(path, **arrays)


def damaged():
    """name -> (bytes, kind, a word of the reason): files PngDecoder.decode must refuse only once it inflates."""
    rng = np.random.RandomState(2605)
    s = rng.randint(0, 256, (6, 5, 3))
    raw = S.scanlines(s, 2, 8, CYCLE)
    bad_filter = bytearray(raw)
    bad_filter[2 * 16] = 5
    z = bytearray(zlib.compress(raw))
    z[-1] ^= 0x55                               # the Adler-32 of the stream
    broken = S.SIGNATURE + S.ihdr(5, 6, 8, 2) + S.chunk(b'IDAT', bytes(z)) + S.chunk(b'IEND')
    return dict(short=(S.make_png(s, 2, 8, stream=raw[:-1]), 'corrupt', 'ends after'),
                long=(S.make_png(s, 2, 8, stream=raw + b'\0'), 'corrupt', 'longer'),
                filter5=(S.make_png(s, 2, 8, stream=bytes(bad_filter)), 'corrupt', 'filter type 5'),
                zlib=(broken, 'corrupt', 'zlib'))


if __name__ == '__main__':
    write_golden(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'g26_png.npz'))
