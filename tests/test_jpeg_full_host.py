"""The host stage under an accept mask (ppy_jpeg_info_ex, ppy_jpeg_entropy_decode_ex; no GPU): progressive files, sequential
files in several scans and the further luma sampling factors.  Three links: Pillow (libjpeg-turbo) == tests/jpeg_full_ref.py
on the goldens of g22_jpeg_full.npz and on a seeded sweep of files written by tests/jpeg_full_synth.py; the restatement's
coefficients == the library's, element for element; and the refusals -- each mask bit lifts its own and no other."""
import ctypes
import struct

import numpy as np
import pytest

import jpeg_fixtures as F20
import jpeg_full_fixtures as F
import jpeg_full_ref as FR
import jpeg_full_synth as FS
import jpeg_ref as R
import jpeg_synth as S

UNSUPPORTED, CORRUPT = -2, -5
P, M, SA = FR.PROGRESSIVE, FR.MULTISCAN, FR.SAMPLING


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from ppyolo_hip import _lib
    return _lib.lib()


def info_of(L, b, accept=FR.ALL):
    from ppyolo_hip import _lib
    info = _lib.JpegInfo()
    rc = L.ppy_jpeg_info_ex(b, len(b), accept, ctypes.byref(info))
    assert rc == info.status
    return rc, info


def decode_of(L, b, coef_bytes, accept=FR.ALL):
    from ppyolo_hip import _lib
    coef = np.full(max(coef_bytes // 2, 1), 0x5a5a, np.int16)          # the call zeroes what it owns
    desc = _lib.JpegDesc()
    desc.coef_base = 4096
    reason = ctypes.create_string_buffer(64)
    rc = L.ppy_jpeg_entropy_decode_ex(b, len(b), accept, coef.ctypes.data, coef_bytes, ctypes.byref(desc), reason)
    return rc, coef, desc, reason.value.decode()


def status_of(L, b, accept):
    """(code, reason) of the two calls in turn, as JpegDecoder makes them."""
    rc, info = info_of(L, b, accept)
    if rc != 0:
        return rc, info.reason.decode()
    rc, _, _, reason = decode_of(L, b, info.coef_bytes, accept)
    return rc, reason


def same_as_restatement(L, b, hd):
    """info, descriptor and every coefficient of the library against the restatement's dict."""
    rc, info = info_of(L, b)
    assert rc == 0 and info.reason == b''
    assert (info.width, info.height, info.components, info.orientation) == (hd['W'], hd['H'], len(hd['comps']), hd['orientation'])
    assert info.progressive == int(hd['progressive'])
    swap = hd['orientation'] >= 5
    assert (info.out_width, info.out_height) == ((hd['H'], hd['W']) if swap else (hd['W'], hd['H']))
    rc, coef, desc, reason = decode_of(L, b, info.coef_bytes)
    assert rc == 0 and reason == '' and desc.coef_base == 4096
    assert (desc.width, desc.height, desc.components, desc.orientation) == (info.width, info.height, info.components, info.orientation)
    off = 0
    for c, comp in enumerate(hd['comps']):
        bh, bw = comp['coef'].shape[:2]
        assert (info.blocks_h[c], info.blocks_w[c], info.h_samp[c], info.v_samp[c]) == (bh, bw, comp['h'], comp['v'])
        assert (desc.blocks_h[c], desc.blocks_w[c], desc.h_samp[c], desc.v_samp[c], desc.coef_offset[c]) == (bh, bw, comp['h'], comp['v'], off)
        mine = coef[off:off + bh * bw * 64].reshape(bh, bw, 8, 8).transpose(0, 1, 3, 2).reshape(bh, bw, 64)
        assert np.array_equal(mine, comp['coef']), (c, int((mine != comp['coef']).sum()))
        assert np.array_equal(np.array(desc.quant[c]).reshape(8, 8).T.reshape(64), hd['q'][comp['tq']])
        off += bh * bw * 64
    assert info.coef_bytes == desc.coef_bytes == off * 2
    assert not (coef[off:] != 0x5a5a).any()


# ------------------------------------------------------------------------------------------------------------- goldens
def test_goldens_hold_what_the_issue_lists():
    names = F.names()
    assert str(F.golden()['pillow']) and len(F.incomplete()) == 2
    for word in ('p444', 'p422', 'p420', 'pgrey', '_q35', '_q75', '_q95', '_dri1', '_dri3', 'orient6', '_1x1', '_7x9', '_17x23', '_37x53',
                 '_300x', 'scans3', 'scans12', 'single', 'default', 'spectral', 'deep', '_3x2', '_5x9', '_40x70') + tuple(FS.NEW_LUMA):
        assert any(word in n for n in names), word
    for n in F20.names():                              # the mask changes nothing about a baseline file
        if n.startswith('coco_'):
            continue
        hd = R.coefficients(F20.data(n))
        got = FR.coefficients(F20.data(n))
        assert all(np.array_equal(a['coef'], b['coef']) for a, b in zip(got['comps'], hd['comps'])) and got['scans'] == 1


@pytest.mark.parametrize('name', F.names())
def test_restatement_equals_the_golden_pixels(name):
    assert F.matches_golden(name, FR.reconstruct(F.coefficients(name)))


@pytest.mark.parametrize('name', F.names())
def test_library_equals_the_restatement_on_goldens(L, name):
    same_as_restatement(L, F.data(name), F.coefficients(name))


def test_progressive_fixture_of_the_baseline_goldens(L):
    b = F20.data('progressive_30x30')
    assert info_of(L, b, 0)[0] == UNSUPPORTED and info_of(L, b, M | SA)[0] == UNSUPPORTED
    hd = FR.coefficients(b)
    assert hd['progressive'] and hd['scans'] > 1
    same_as_restatement(L, b, hd)


# --------------------------------------------------------------------------------------------------------------- sweep
SWEEP_SIZES = [(1, 1), (2, 3), (9, 5), (17, 17), (23, 40)]             # (H, W)
LUMAS = dict(FS.NEW_LUMA, **{'444': (1, 1), '422': (2, 1), '420': (2, 2), 'grey': 'grey'})


def sweep_files():
    """Samplings x scripts x sizes x restart intervals x orientations, every axis cycling against the others -> [(key, file,
    dict the file was written from)]; built once."""
    if not _SWEEP:
        rng = np.random.default_rng(2200)
        k = 0
        stats = {}
        for lname, luma in LUMAS.items():
            for H, W in SWEEP_SIZES:
                for kind in ('single', 'scans3', 'scans12', 'default', 'spectral', 'deep'):
                    hd = FS.synth(rng, H, W, luma, orientation=1 + k % 8)
                    n = len(hd['comps'])
                    dri, tables = (0, 1, 3)[(k // 6 + k) % 3], ('flat', 'skewed')[k // 6 % 2]
                    k += 1
                    if kind == 'single':
                        b = S.encode(hd, dri=dri, tables=tables)
                    elif kind.startswith('scans'):
                        if n == 1:
                            continue
                        FS.clear_padding(hd)
                        groups = [[1], [0], [2]] if kind == 'scans3' else [[0], [2, 1]] if k % 2 else [[1, 2], [0]]
                        b = FS.sequential(hd, groups, dri=[dri, 0, 3][:len(groups)] if k % 3 == 0 else dri, tables=tables)
                    else:
                        FS.clear_padding(hd)
                        b = FS.progressive(hd, FS.SCRIPTS[kind](n), dri=dri, tables=tables, stats=stats if dri == 0 else None,
                                           late_tables=k % 2 == 0)
                    _SWEEP.append(((lname, H, W, kind, dri, tables, hd['orientation']), b, hd))
        _SWEEP_STATS.update(stats)
    return _SWEEP


_SWEEP, _SWEEP_STATS = [], {}


def test_sweep_reaches_the_traps():
    files = sweep_files()
    assert len(files) > 300
    assert _SWEEP_STATS['eobrun_max'] > 5                                         # longer than the 5 block columns of a 40-wide row
    assert all(_SWEEP_STATS.get('len%d' % n, 0) > 0 for n in range(10, 17))       # codes past the 9-bit lookahead
    keys = [k for k, _, _ in files]
    assert any(k[0] == '420' and k[2] == 17 and k[3] in ('default', 'scans3') for k in keys)          # 3 real luma block columns of 4
    assert any(k[0] == '411' and k[2] == 5 for k in keys) and any(k[0] == '440' and k[1] <= 2 for k in keys)
    assert {k[4] for k in keys if k[3] in ('default', 'spectral', 'deep')} == {0, 1, 3}
    assert {k[6] for k in keys} == set(range(1, 9))


def test_restatement_equals_pillow_on_goldens_and_sweep():
    from PIL import Image  # noqa: F401         a plain import: without Pillow this pin fails, it does not skip
    for name in F.names():
        assert np.array_equal(FR.reconstruct(F.coefficients(name)), S.pillow_pixels(F.data(name))), name
    for key, b, hd in sweep_files():
        got = FR.coefficients(b)
        assert all(np.array_equal(a['coef'], c['coef']) for a, c in zip(got['comps'], hd['comps'])), key
        assert np.array_equal(FR.reconstruct(got), S.pillow_pixels(b)), key


def test_library_equals_the_restatement_on_the_sweep(L):
    for key, b, hd in sweep_files():
        same_as_restatement(L, b, FR.coefficients(b))


# ------------------------------------------------------------------------------------------------------------ refusals
def _files_by_need():
    rng = np.random.default_rng(2201)
    y420, y440 = FS.clear_padding(FS.synth(rng, 17, 17, (2, 2))), FS.clear_padding(FS.synth(rng, 9, 5, (1, 2)))
    return [(P, FS.progressive(y420, FS.script_default(3)), 'progressive'),
            (M, FS.sequential(y420, [[0], [1], [2]]), 'multiple scans'),
            (M, FS.sequential(y420, [[1, 0, 2]]), 'scan component order'),
            (SA, S.encode(y440), 'sampling'),
            (P | SA, FS.progressive(y440, FS.script_spectral(3)), None),
            (M | SA, FS.sequential(y440, [[0], [1, 2]]), None)]


def test_each_mask_bit_lifts_its_own_refusal_and_no_other(L):
    for need, b, word in _files_by_need():
        hd = FR.coefficients(b)
        for accept in range(8):
            rc, reason = status_of(L, b, accept)
            if accept & need == need:
                assert (rc, reason) == (0, ''), (need, accept, reason)
                same = decode_of(L, b, info_of(L, b, accept)[1].coef_bytes, accept)[1]
                assert np.array_equal(same, decode_of(L, b, info_of(L, b)[1].coef_bytes)[1])
            else:
                assert rc == UNSUPPORTED, (need, accept, rc, reason)
                if word and accept == 0:
                    assert word in reason
                try:
                    FR.coefficients(b, accept)
                    raise AssertionError('the restatement accepted it')
                except R.JpegUnsupported:
                    pass
        assert hd['scans'] >= 1
    # what no bit lifts: chroma factors other than 1x1, more than 10 blocks in an MCU, arithmetic coding, 12 bits
    rng = np.random.default_rng(2202)
    hd = FS.synth(rng, 9, 9, (2, 2))
    b = S.encode(hd)
    sof = b.index(b'\xff\xc0')
    cases = [b[:sof + 14] + b'\x21' + b[sof + 15:], b[:sof + 11] + b'\x43' + b[sof + 12:], b[:sof + 1] + b'\xc9' + b[sof + 2:],
             b[:sof + 4] + b'\x0c' + b[sof + 5:]]
    for bad in cases:
        assert status_of(L, bad, FR.ALL)[0] == UNSUPPORTED
    assert L.ppy_jpeg_info_ex(b, len(b), 8, ctypes.byref(info_of(L, b)[1])) == -1          # an unknown bit is a bad argument


def test_mask_zero_is_the_old_entry_point(L):
    from ppyolo_hip import _lib
    for b in [F20.data(n) for n in F20.names()[:6]] + [F20.data('progressive_30x30'), F20.data('truncated_c420_37x53'), b'', b'\xff\xd8\xff']:
        a, c = _lib.JpegInfo(), _lib.JpegInfo()
        assert L.ppy_jpeg_info(b, len(b), ctypes.byref(a)) == L.ppy_jpeg_info_ex(b, len(b), 0, ctypes.byref(c))
        assert bytes(a) == bytes(c)


def test_incomplete_script_is_unsupported(L):
    for name in F.incomplete():
        rc, reason = status_of(L, F.data(name), FR.ALL)
        assert rc == UNSUPPORTED and 'incomplete progressive scan script' in reason
        with pytest.raises(R.JpegUnsupported):
            FR.coefficients(F.data(name))


def _patch_sos(b, k, **kw):
    """The file with fields of its k-th SOS segment replaced."""
    b = bytearray(b)
    i = -1
    for _ in range(k + 1):
        i = b.index(b'\xff\xda', i + 1)
    ns = b[i + 4]
    t = i + 5 + 2 * ns
    for key, at in (('ss', t), ('se', t + 1), ('ahal', t + 2), ('ns', i + 4), ('id0', i + 5)):
        if key in kw:
            b[at] = kw[key]
    return bytes(b)


def test_illegal_scan_parameters_are_corrupt(L):
    rng = np.random.default_rng(2203)
    hd = FS.clear_padding(FS.synth(rng, 17, 23, (2, 2)))
    b = FS.progressive(hd, FS.script_default(3), late_tables=False)
    assert status_of(L, b, FR.ALL) == (0, '')
    seq = FS.sequential(hd, [[0], [1], [2]])
    eoi = b.rindex(b'\xff\xd9')
    sos2 = b.index(b'\xff\xda', b.index(b'\xff\xda') + 1)
    first_dht = b.index(b'\xff\xc4')
    cases = {
        'Ss past 63': _patch_sos(b, 1, ss=64), 'Se below Ss': _patch_sos(b, 1, ss=6, se=5), 'Al past 13': _patch_sos(b, 1, ahal=0x0e),
        'DC scan with Se != 0': _patch_sos(b, 0, se=5),
        'AC scan with two components': b[:sos2] + b'\xff\xda' + struct.pack('>H', 10) + bytes([2, 1, 0, 2, 0x11, 1, 5, 2]) + b[sos2 + 10:],
        'refinement with Ah != Al + 1': _patch_sos(b, 5, ahal=0x20),
        'unknown component': _patch_sos(b, 1, id0=9), 'component twice': _twice(b),
        'sequential component repeated': _patch_sos(seq, 1, id0=1),
        'missing table': b[:first_dht] + b[first_dht + 2 + (b[first_dht + 2] << 8 | b[first_dht + 3]):],
        'data ends early': b[:sos2 + 12] + b[eoi:], 'no EOI': b[:eoi], 'out of order': _patch_sos(b, 1, ahal=0x21),
    }
    for what, bad in cases.items():
        rc, reason = status_of(L, bad, FR.ALL)
        assert rc == CORRUPT and reason, (what, rc, reason)
        with pytest.raises(R.JpegCorrupt):
            FR.coefficients(bad)
    # more than 256 scans, every one of them legal: one coefficient per scan, then refinements
    grey = FS.clear_padding(FS.synth(rng, 8, 8, 'grey'))
    script = [((0,), 0, 0, 0, 0)] + [((0,), k, k, 0, 13) for k in range(1, 64)]
    for a in range(13, 9, -1):
        script += [((0,), k, k, a, a - 1) for k in range(1, 64)]
    assert len(script) > 256
    rc, reason = status_of(L, FS.progressive(grey, script), FR.ALL)
    assert rc == UNSUPPORTED and '256' in reason


def _twice(b):
    """The first (interleaved DC) scan naming component 1 twice."""
    b = bytearray(b)
    i = b.index(b'\xff\xda')
    b[i + 7] = b[i + 5]
    return bytes(b)


# ------------------------------------------------------------------------------------------------------------ prefixes
@pytest.mark.parametrize('name', ['pil_p420_q75_dri1_17x23', 'pil_pgrey_q75_dri1_7x9', 'syn_1x4_deep_dri1_5x9'])
def test_every_prefix_returns_a_status(L, name):
    """Every strict prefix of three progressive goldens: corrupt under the mask (without it: today's codes, corrupt until the
    SOF2 marker is whole and unsupported from there on), never a crash or a hang; only the whole file decodes."""
    b = F.data(name)
    assert FR.coefficients(b)['progressive']
    rc, info = info_of(L, b)
    full = info.coef_bytes
    assert decode_of(L, b, full)[0] == 0
    for n in range(len(b)):
        pre = bytes(b[:n])                   # an exact-size copy
        rc, info = info_of(L, pre)
        assert rc in (0, CORRUPT), (n, rc)
        assert info_of(L, pre, 0)[0] in (CORRUPT, UNSUPPORTED)
        if rc == 0:
            assert info.coef_bytes == full
            rc = decode_of(L, pre, full)[0]
            assert rc == CORRUPT, (n, rc)
