"""Host stage of the JPEG decoder through the C ABI (no GPU): ppy_jpeg_info, ppy_jpeg_entropy_decode and the descriptor
table, against tests/jpeg_ref.py on every fixture of tests/golden/g20_jpeg.npz; refusals; and a prefix sweep (no input may
crash the library)."""
import ctypes
import struct
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import jpeg_fixtures as F
import jpeg_ref as R

UNSUPPORTED, CORRUPT = -2, -5


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from ppyolo_hip import _lib
    return _lib.lib()


def info_of(L, b):
    from ppyolo_hip import _lib
    info = _lib.JpegInfo()
    rc = L.ppy_jpeg_info(b, len(b), ctypes.byref(info))
    assert rc == info.status
    return rc, info


def decode_of(L, b, coef_bytes):
    from ppyolo_hip import _lib
    coef = np.full(max(coef_bytes // 2, 1), 0x5a5a, np.int16)          # the call zeroes what it owns
    desc = _lib.JpegDesc()
    desc.coef_base = 4096
    reason = ctypes.create_string_buffer(64)
    rc = L.ppy_jpeg_entropy_decode(b, len(b), coef.ctypes.data, coef_bytes, ctypes.byref(desc), reason)
    return rc, coef, desc, reason.value.decode()


@pytest.mark.parametrize('name', F.names())
def test_info_and_coefficients(L, name):
    b = F.data(name)
    hd = R.coefficients(b)
    rc, info = info_of(L, b)
    assert rc == 0 and info.reason == b''
    assert (info.width, info.height, info.components, info.orientation) == (hd['W'], hd['H'], len(hd['comps']), hd['orientation'])
    swap = hd['orientation'] >= 5
    assert (info.out_width, info.out_height) == ((hd['H'], hd['W']) if swap else (hd['W'], hd['H']))
    assert info.restart_interval == hd['dri']
    total = 0
    for c, comp in enumerate(hd['comps']):
        assert (info.h_samp[c], info.v_samp[c]) == (comp['h'], comp['v'])
        assert (info.blocks_h[c], info.blocks_w[c]) == comp['coef'].shape[:2]
        total += comp['coef'].size * 2
    assert info.coef_bytes == total
    rc, coef, desc, reason = decode_of(L, b, info.coef_bytes)
    assert rc == 0 and reason == '' and desc.coef_base == 4096 and desc.coef_bytes == total
    assert (desc.width, desc.height, desc.components, desc.orientation) == (info.width, info.height, info.components, info.orientation)
    for c, comp in enumerate(hd['comps']):
        bh, bw = comp['coef'].shape[:2]
        assert (desc.blocks_h[c], desc.blocks_w[c], desc.h_samp[c], desc.v_samp[c]) == (bh, bw, comp['h'], comp['v'])
        mine = coef[desc.coef_offset[c]:desc.coef_offset[c] + bh * bw * 64].reshape(bh, bw, 8, 8)
        assert np.array_equal(mine.transpose(0, 1, 3, 2).reshape(bh, bw, 64), comp['coef'])        # stored column-major in a block
        assert np.array_equal(np.array(desc.quant[c]).reshape(8, 8).T.reshape(64), hd['q'][comp['tq']])


@pytest.mark.parametrize('name,kind', F.refused())
def test_refusals_of_the_fixtures(L, name, kind):
    b = F.data(name)
    rc, info = info_of(L, b)
    if kind == 'unsupported':
        assert rc == UNSUPPORTED and b'progressive' in info.reason
        assert decode_of(L, b, 1 << 16)[0] == UNSUPPORTED
    else:
        assert rc == 0                                          # the header is whole; the entropy data is not
        rc, _, _, reason = decode_of(L, b, info.coef_bytes)
        assert rc == CORRUPT and 'ends early' in reason
    assert L.ppy_error_string(CORRUPT).decode().startswith('corrupt')


def _patch_sof(b, **kw):
    """The file with fields of its SOF segment replaced: marker, precision, ncomp, samp0 (h << 4 | v of component 0)."""
    b = bytearray(b)
    i = 2
    while b[i + 1] not in (0xC0, 0xC1):
        i += 2 + (b[i + 2] << 8 | b[i + 3])
    if 'marker' in kw:
        b[i + 1] = kw['marker']
    if 'precision' in kw:
        b[i + 4] = kw['precision']
    if 'samp0' in kw:
        b[i + 11] = kw['samp0']
    return bytes(b)


def test_unsupported_and_corrupt_codes(L):
    base = F.data('c420_37x53')
    cases = [(_patch_sof(base, marker=0xC2), UNSUPPORTED, 'progressive'), (_patch_sof(base, marker=0xC9), UNSUPPORTED, 'arithmetic'),
             (_patch_sof(base, marker=0xC3), UNSUPPORTED, 'lossless'), (_patch_sof(base, precision=12), UNSUPPORTED, 'precision'),
             (_patch_sof(base, samp0=0x12), UNSUPPORTED, 'sampling'), (_patch_sof(base, samp0=0x41), UNSUPPORTED, 'sampling'),
             (b'', CORRUPT, 'SOI'), (b'\x89PNG\r\n\x1a\n' + bytes(32), CORRUPT, 'SOI'), (base[:2] + b'\xff\xd9', CORRUPT, 'marker'),
             (base[:200], CORRUPT, '')]
    adobe = b'\xff\xee' + struct.pack('>H', 14) + b'Adobe' + bytes([0, 100, 0, 0, 0, 0, 0])          # transform 0 = RGB
    cases.append((base[:2] + adobe + base[2:], UNSUPPORTED, 'Adobe'))
    sos = base.index(b'\xff\xda')
    assert base[sos + 4] == 3
    one_comp_scan = base[:sos] + b'\xff\xda' + struct.pack('>H', 8) + bytes([1, base[sos + 5], base[sos + 6], 0, 63, 0]) + base[sos + 14:]
    cases.append((one_comp_scan, UNSUPPORTED, 'multiple scans'))
    for b, want, word in cases:
        rc, info = info_of(L, b)
        assert rc == want and word in info.reason.decode(), (rc, info.reason, want, word)
    # damaged entropy data: a marker in the middle of it; a wrong restart number; a missing Huffman table
    hd = R.parse(base)
    mid = hd['data'] + (len(base) - hd['data']) // 2
    rc, info = info_of(L, base)
    assert decode_of(L, base[:mid] + b'\xff\xd9' + base[mid:], info.coef_bytes)[0] == CORRUPT
    dri = F.data('c420_dri_65x33')
    k = dri.index(b'\xff\xd1', R.parse(dri)['data'])
    assert decode_of(L, dri[:k] + b'\xff\xd3' + dri[k + 2:], info_of(L, dri)[1].coef_bytes)[0] == CORRUPT
    dht = base.index(b'\xff\xc4')
    n = 2 + (base[dht + 2] << 8 | base[dht + 3])
    assert info_of(L, base[:dht] + base[dht + n:])[0] == CORRUPT
    # a too small coefficient buffer is refused, not overrun
    assert decode_of(L, base, info.coef_bytes - 128)[0] == -3


@pytest.mark.parametrize('name,stride', [('c420_dri_65x33', 1), ('c444_q16big_20x27', 1), ('segments_33x35', 1), ('coco_398725', 97)])
def test_every_prefix_returns_a_status(L, name, stride):
    """Prefixes at a fixed stride of lengths (every length for the small files): a status code, never a crash; only the
    whole entropy data decodes."""
    b = F.data(name)
    rc, info = info_of(L, b)
    full = info.coef_bytes
    want = decode_of(L, b, full)[1]
    oks = 0
    for n in list(range(0, len(b), stride)) + [len(b)]:
        pre = bytes(b[:n])                   # an exact-size copy: an over-read would be the allocator's to catch under ASan
        rc, info = info_of(L, pre)
        assert rc in (0, CORRUPT), (n, rc)
        if rc == 0:
            assert info.coef_bytes == full
            rc, coef, _, _ = decode_of(L, pre, full)
            assert rc in (0, CORRUPT), (n, rc)
            if rc == 0:
                oks += 1
                assert np.array_equal(coef, want), n
    assert 1 <= oks <= 2 + 8 // stride          # the whole file, and the file less (part of) its EOI marker and pad bits


def test_byte_flips_never_crash(L):
    """Every byte of a small file replaced by 0x00 / 0xFF / its complement: a status code each time."""
    b = F.data('c422_dri_opt_41x70')
    seen = set()
    for i in range(len(b)):
        for v in (0, 0xFF, b[i] ^ 0xFF):
            m = b[:i] + bytes([v]) + b[i + 1:]
            rc, info = info_of(L, m)
            if rc == 0 and info.coef_bytes <= 1 << 24:
                rc = decode_of(L, m, info.coef_bytes)[0]
            seen.add(rc)
            assert rc in (0, UNSUPPORTED, CORRUPT), (i, v, rc)
    assert seen == {0, UNSUPPORTED, CORRUPT}


def test_entropy_stage_is_thread_safe(L):
    names = F.names() * 4
    serial = [decode_of(L, F.data(n), info_of(L, F.data(n))[1].coef_bytes)[1] for n in names]
    with ThreadPoolExecutor(max_workers=8) as pool:
        par = list(pool.map(lambda n: decode_of(L, F.data(n), info_of(L, F.data(n))[1].coef_bytes)[1], names))
    assert all(np.array_equal(a, b) for a, b in zip(serial, par))


def test_table_and_workspace(L):
    """ppy_jpeg_pack_table / ppy_jpeg_workspace_bytes are host arithmetic: sizes, and refusal of a descriptor that does not
    describe its own geometry."""
    from ppyolo_hip import _lib
    names = ['c420_37x53', 'grey_29x43', 'orient6_21x13']
    descs = (_lib.JpegDesc * 3)()
    base = 0
    for i, n in enumerate(names):
        b = F.data(n)
        rc, coef, d, _ = decode_of(L, b, info_of(L, b)[1].coef_bytes)
        assert rc == 0
        d.coef_base = base
        base += d.coef_bytes
        descs[i] = d
    planes = sum(d.blocks_w[c] * d.blocks_h[c] * 64 for d in descs for c in range(d.components))
    assert L.ppy_jpeg_workspace_bytes(3, descs) == planes and L.ppy_jpeg_table_bytes(3) % 16 == 0
    tb = L.ppy_jpeg_table_bytes(3)
    table = np.zeros(tb, np.uint8)
    outs = (ctypes.c_void_p * 3)(0x1000, 0x2000, 0x3000)
    ok = (ctypes.c_longlong * 3)(3 * 53, 3 * 43, 3 * 21)
    assert L.ppy_jpeg_pack_table(3, descs, outs, ok, 1, table.ctypes.data, tb) == 0
    tight = (ctypes.c_longlong * 3)(3 * 53, 3 * 43, 3 * 13)          # image 2 is stored 13 wide and displayed 21 wide
    assert L.ppy_jpeg_pack_table(3, descs, outs, tight, 0, table.ctypes.data, tb) == 0
    assert L.ppy_jpeg_pack_table(3, descs, outs, tight, 1, table.ctypes.data, tb) == -1
    assert L.ppy_jpeg_pack_table(3, descs, outs, ok, 1, table.ctypes.data, tb - 1) == -1
    descs[1].blocks_w[0] += 1
    assert L.ppy_jpeg_workspace_bytes(3, descs) == 0
    assert L.ppy_jpeg_pack_table(3, descs, outs, ok, 1, table.ctypes.data, tb) == -1
