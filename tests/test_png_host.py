"""The host side of PNG decoding, without a GPU and without the library: the numpy restatement (tests/png_ref.py) against the
installed Pillow, the chunk walk of ppyolo_hip/png.py, every refusal by kind and reason, and ImageDecoder's sniffing and index
mapping with stub decoders."""
import io
import struct
import warnings
import zlib

import numpy as np
import pytest

import png_cases as C
import png_ref
import png_synth as S
from ppyolo_hip import png
from ppyolo_hip._lib import PPYoloHipError
from ppyolo_hip.imagefile import ImageDecoder, sniff


def pillow(data):
    from PIL import Image
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        return np.asarray(Image.open(io.BytesIO(data)).convert('RGB'))[..., ::-1]


def test_restatement_equals_pillow_on_every_case_but_grey16():
    """Bit for bit on every synthesised file; 16-bit grey without alpha is the named exception: there the restatement keeps the
    high byte, and Pillow (mode I;16, convert('RGB') clips to 255) really does differ."""
    cases = C.all_cases()
    assert len(cases) > 200
    differs = 0
    for name, data in cases.items():
        if C.is_grey16(data):
            continue
        assert np.array_equal(C.want(name), pillow(data)), name
    rng = np.random.RandomState(7)
    s = rng.randint(256, 65536, (5, 7, 1))
    for interlace in (0, 1):
        data = S.make_png(s, 0, 16, C.CYCLE, interlace)
        assert C.is_grey16(data)
        got = png_ref.decode(data)
        assert np.array_equal(got, np.repeat((s >> 8).astype(np.uint8), 3, -1))
        differs += int(not np.array_equal(got, pillow(data)))
    assert differs == 2, 'Pillow no longer departs from the high-byte rule on 16-bit grey: pin that case to Pillow as well'


def test_golden_file_is_what_the_cases_give():
    g = C.golden()
    assert [str(n) for n in g['names']] == C.GOLDEN
    for n in C.GOLDEN:
        assert g['png_' + n].tobytes() == C.all_cases()[n], n
        assert np.array_equal(g['bgr_' + n], C.want(n)), n
        if not C.is_grey16(C.all_cases()[n]):
            assert np.array_equal(g['bgr_' + n], pillow(C.all_cases()[n])), (n, 'installed Pillow')


def test_palette_index_past_plte_is_black_as_in_pillow():
    data = C.all_cases()['pal_short']
    want = C.want('pal_short')
    idx = png_ref.unfilter(zlib.decompress(b''.join(b for t, b in png_ref.chunks(data) if t == b'IDAT')), 4, 9, 1)
    assert (idx >= 5).any() and np.all(want[idx >= 5] == 0) and np.array_equal(want, pillow(data))


# ---- the chunk walk -----------------------------------------------------------------------------------------------------------
RGB = np.random.RandomState(11).randint(0, 256, (6, 5, 3))


def test_expected_length_formula():
    assert png.expected_bytes(5, 6, 2, 8, 0) == 6 * 16
    assert png.expected_bytes(1, 1, 0, 1, 1) == 2                                  # six empty passes
    assert [p[4:6] for p in png.passes(3, 2, 2, 8, 1)] == [(1, 1), (1, 1), (1, 1), (3, 1)]      # passes 1, 2 and 4 are empty
    assert png.expected_bytes(3, 2, 2, 8, 1) == 4 + 4 + 4 + 10
    assert png.expected_bytes(9, 5, 0, 2, 1) == sum(r * (1 + (c * 2 + 7) // 8) for c, r in ((2, 1), (1, 1), (3, 1), (2, 2), (5, 1), (4, 3), (9, 2)))
    for name, data in C.all_cases().items():
        h = png.parse(data)
        assert h.expected == len(zlib.decompress(b''.join(bytes(b) for b in h.idat))), name


def test_idat_split_empty_and_inside_the_zlib_header():
    one = png.inflate(png.parse(S.make_png(RGB, 2, 8, C.CYCLE)))
    for sizes in ([1], [0, 1, 0, 1, 0, 3], [0], [2, 7, 0, 0, 11]):
        h = png.parse(S.make_png(RGB, 2, 8, C.CYCLE, idat_sizes=sizes))
        assert len(h.idat) == len(sizes) + 1 and png.inflate(h) == one, sizes


def test_ancillary_and_apng_chunks_are_skipped_and_bytes_after_iend_ignored():
    plain = S.make_png(RGB, 2, 8, C.CYCLE)
    before = [S.chunk(t, b) for t, b in ((b'gAMA', struct.pack('>I', 45455)), (b'sRGB', b'\0'), (b'cHRM', bytes(32)), (b'pHYs', bytes(9)),
                                         (b'bKGD', bytes(6)), (b'tEXt', b'k\0v'), (b'tIME', bytes(7)), (b'iCCP', b'n\0\0' + zlib.compress(b'x')),
                                         (b'acTL', bytes(8)), (b'fcTL', bytes(26)), (b'tRNS', bytes(6)))]
    after = [S.chunk(b'fcTL', bytes(26)), S.chunk(b'fdAT', bytes(4) + zlib.compress(bytes(96))), S.chunk(b'tEXt', b'k\0v')]
    busy = S.make_png(RGB, 2, 8, C.CYCLE, before_idat=before, after_idat=after, tail=b'trailing bytes')
    a, b = png.parse(plain), png.parse(busy)
    assert a[:6] == b[:6] and png.inflate(a) == png.inflate(b)
    assert png.PngDecoder(device='cpu').refusal(busy) is None


def refusal(data, **kw):
    return png.PngDecoder(device='cpu', **kw).refusal(data)


def _with_ihdr(**kw):
    f = dict(width=5, height=6, depth=8, ctype=2, interlace=0, compression=0, filter_method=0)
    f.update(kw)
    z = zlib.compress(S.scanlines(RGB, 2, 8))
    return S.SIGNATURE + S.ihdr(f['width'], f['height'], f['depth'], f['ctype'], f['interlace'], f['compression'], f['filter_method']) + \
        S.chunk(b'IDAT', z) + S.chunk(b'IEND')


def _bad_crc(data, ctype):
    at = data.index(ctype) + 4 + int.from_bytes(data[data.index(ctype) - 4:data.index(ctype)], 'big')
    return data[:at] + bytes([data[at] ^ 1]) + data[at + 1:]


PAL = S.make_png(np.zeros((2, 2, 1), int), 3, 8, palette=bytes(6))
REFUSALS = [
    ('bad signature', b'\x89PNG\r\n\x1a\r' + _with_ihdr()[8:], 'corrupt', 'bad signature'),
    ('empty', b'', 'corrupt', 'bad signature'),
    ('crc ihdr', _bad_crc(_with_ihdr(), b'IHDR'), 'corrupt', 'bad CRC in chunk IHDR'),
    ('crc plte', _bad_crc(PAL, b'PLTE'), 'corrupt', 'bad CRC in chunk PLTE'),
    ('crc idat', _bad_crc(_with_ihdr(), b'IDAT'), 'corrupt', 'bad CRC in chunk IDAT'),
    ('truncated in idat', _with_ihdr()[:60], 'corrupt', 'truncated: chunk IDAT'),
    ('truncated header', _with_ihdr()[:37], 'corrupt', 'truncated inside a chunk header'),
    ('no iend', _with_ihdr()[:-12], 'corrupt', 'truncated: no IEND'),
    ('zero width', _with_ihdr(width=0), 'corrupt', 'width 0'),
    ('depth 3', _with_ihdr(depth=3), 'corrupt', 'bit depth 3'),
    ('colour type 5', _with_ihdr(ctype=5), 'corrupt', 'colour type 5'),
    ('16-bit palette', _with_ihdr(ctype=3, depth=16), 'corrupt', 'bit depth 16 with colour type 3'),
    ('missing plte', _with_ihdr(ctype=3), 'corrupt', 'missing PLTE'),
    ('plte of 7 bytes', S.make_png(np.zeros((2, 2, 1), int), 3, 8, palette=bytes(7)), 'corrupt', 'PLTE of 7 bytes'),
    ('plte of 771 bytes', S.make_png(np.zeros((2, 2, 1), int), 3, 8, palette=bytes(771)), 'corrupt', 'PLTE of 771 bytes'),
    ('unknown critical', S.make_png(RGB, 2, 8, before_idat=[S.chunk(b'CgBI', bytes(4))]), 'unsupported', 'unknown critical chunk CgBI'),
    ('interlace 2', _with_ihdr(interlace=2), 'unsupported', 'interlace method 2'),
    ('compression 1', _with_ihdr(compression=1), 'unsupported', 'compression method 1'),
    ('filter method 1', _with_ihdr(filter_method=1), 'unsupported', 'filter method 1'),
    ('side over 65535', _with_ihdr(width=65536), 'unsupported', 'a side is over 65535'),
    ('ihdr not first', S.SIGNATURE + S.chunk(b'gAMA', bytes(4)) + _with_ihdr()[8:], 'corrupt', 'the first chunk is gAMA, not IHDR'),
    ('plte after idat', S.make_png(np.zeros((2, 2, 1), int), 3, 8, palette=bytes(6), after_idat=[S.chunk(b'PLTE', bytes(6))]), 'corrupt',
     'a second PLTE'),
    ('idat not consecutive', S.make_png(RGB, 2, 8, after_idat=[S.chunk(b'tEXt', b'k\0v'), S.chunk(b'IDAT', b'')]), 'corrupt',
     'IDAT chunks are not consecutive'),
    ('no idat', S.SIGNATURE + S.ihdr(5, 6, 8, 2) + S.chunk(b'IEND'), 'corrupt', 'no IDAT'),
]


@pytest.mark.parametrize('case', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusal_by_kind_and_reason(case):
    _, data, kind, reason = case
    got = refusal(data)
    assert got is not None and got[0] == kind and reason in got[1], got
    with pytest.raises(PPYoloHipError, match=r'item 0: %s PNG: ' % kind):
        png.PngDecoder(device='cpu').host_decode([data])


def test_a_60_byte_file_that_claims_65535_squared_is_refused_before_any_allocation(monkeypatch):
    data = S.SIGNATURE + S.ihdr(65535, 65535, 16, 6) + S.chunk(b'IDAT', b'\x78\x9c\x03') + S.chunk(b'IEND')
    assert len(data) <= 60 + 8
    dec = png.PngDecoder(device='cpu')
    monkeypatch.setattr(dec, '_staging', lambda nbytes: pytest.fail('a staging buffer of %d bytes was asked for' % nbytes))
    assert dec.refusal(data) == ('unsupported', '65535 x 65535 pixels is over max_pixels = %d' % (1 << 28))
    with pytest.raises(PPYoloHipError, match='item 0: unsupported PNG: 65535 x 65535 pixels is over max_pixels'):
        dec.host_decode([data])
    assert png.PngDecoder(device='cpu', max_pixels=29).refusal(_with_ihdr())[0] == 'unsupported'
    assert png.PngDecoder(device='cpu', max_pixels=30).refusal(_with_ihdr()) is None


def test_inflate_is_bounded_and_its_damage_is_named():
    for name, (data, kind, word) in C.damaged().items():
        h = png.parse(data)                                                        # the chunk walk cannot see it
        with pytest.raises(png.Refusal, match=word) as e:
            png.check_filters(png.inflate(h), h)
        assert e.value.kind == kind, name
        with pytest.raises(PPYoloHipError, match='item 1: corrupt PNG: '):
            png.PngDecoder(device='cpu').host_decode([C.all_cases()['fmt_c2_d8'], data])
    bomb = S.SIGNATURE + S.ihdr(5, 6, 8, 2) + S.chunk(b'IDAT', zlib.compress(bytes(1 << 24))) + S.chunk(b'IEND')
    h = png.parse(bomb)
    got = zlib.decompressobj().decompress(b''.join(bytes(b) for b in h.idat), h.expected + 1)
    assert len(got) == h.expected + 1                                              # what inflate() lets zlib write, whatever the file holds
    with pytest.raises(png.Refusal, match='longer than the 96 bytes'):
        png.inflate(h)


def test_threads_are_capped_and_never_taken_from_the_cpu_count():
    assert png.PngDecoder(device='cpu', threads=64).threads == 16 and png.PngDecoder(device='cpu').threads is None
    assert png.MAX_THREADS == 16
    with pytest.raises(PPYoloHipError):
        png.PngDecoder(device='cpu', threads=0)


# ---- ImageDecoder ---------------------------------------------------------------------------------------------------------------
class Stub(object):
    def __init__(self, kind, fail_at=None):
        self.kind, self.calls, self.fail_at = kind, [], fail_at

    def refusal(self, data):
        return ('corrupt', self.kind + ' says no') if data.endswith(b'bad') else None

    def decode(self, items, out=None):
        self.calls.append(list(items))
        if self.fail_at is not None:
            raise PPYoloHipError('item %d: corrupt %s: stub' % (self.fail_at, self.kind))
        return [(self.kind, bytes(d)) for d in items]


def test_image_decoder_sniffs_splits_and_maps_indices_back():
    J, P = b'\xff\xd8\xff\xe0', S.SIGNATURE
    assert sniff(J + b'x') == 'jpeg' and sniff(P + b'x') == 'png' and sniff(b'BM' + bytes(20)) is None and sniff(b'') is None
    items = [J + b'0', P + b'1', P + b'2', J + b'3', P + b'4']
    jd, pd = Stub('JPEG'), Stub('PNG')
    got = ImageDecoder(jpeg=jd, png=pd).decode(items)
    assert got == [('JPEG', items[0]), ('PNG', items[1]), ('PNG', items[2]), ('JPEG', items[3]), ('PNG', items[4])]
    assert jd.calls == [[items[0], items[3]]] and pd.calls == [[items[1], items[2], items[4]]]       # one decode() call each
    with pytest.raises(PPYoloHipError, match=r'^item 4: corrupt PNG: stub'):
        ImageDecoder(jpeg=Stub('JPEG'), png=Stub('PNG', fail_at=2)).decode(items)
    with pytest.raises(PPYoloHipError, match=r'^item 3: corrupt JPEG: stub'):
        ImageDecoder(jpeg=Stub('JPEG', fail_at=1), png=Stub('PNG')).decode(items)
    d = ImageDecoder(jpeg=Stub('JPEG'), png=Stub('PNG'))
    assert d.refusal(items[0]) is None and d.refusal(P + b'bad') == ('corrupt', 'PNG says no') and d.refusal(J + b'bad') == ('corrupt', 'JPEG says no')
    kind, reason = d.refusal(b'GIF89a' + bytes(10))
    assert kind == 'unsupported' and reason == 'neither a JPEG nor a PNG file (first bytes 4749463839610000)'
    with pytest.raises(PPYoloHipError, match=r'^item 1: .*neither a JPEG nor a PNG file'):
        d.decode([items[0], b'GIF89a' + bytes(10)])
    assert d.imdecode(items[1]) == ('PNG', items[1])


def test_image_decoder_in_decode_records_names_the_record():
    """augment.decode_records with decoder=ImageDecoder(): the refusal pass and the 'item i:' mapping reach the record; the
    message keeps decode_records' own wording."""
    from ppyolo_hip.augment import decode_records
    good, bad = C.all_cases()['fmt_c2_d8'], _with_ihdr(depth=3)
    d = ImageDecoder(jpeg=Stub('JPEG'), png=png.PngDecoder(device='cpu'))
    with pytest.raises(PPYoloHipError, match=r'record 1: corrupt JPEG: bit depth 3'):
        decode_records([dict(image=good), dict(image=bad)], d)
