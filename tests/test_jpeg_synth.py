"""The JPEG decoder on inputs made at the coefficient level (tests/jpeg_synth.py), on the CPU: the encoder and the
restatement's entropy decoder against each other, the library's host stage on streams and Huffman tables that no encoder
library wrote, and the three zones of the inverse DCT (jpeg_synth.py's docstring) pinned to what
each can be pinned to.  Array equality everywhere.  Pillow is needed (a plain import: without it the pins fail)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import jpeg_ref as R
import jpeg_synth as S

SIZES = [(1, 1), (3, 5), (17, 9), (33, 65), (40, 300)]          # (H, W)
DRIS = (0, 1, 3, 9)
_FILES = {}


def files(regime):
    """The matrix for one regime: every sampling x SIZES x DRIS x both table sets, each file with coefficients of its own
    and the orientations in turn -> [(key, hd, dri, tables, bytes)], and the counts of the Huffman code lengths written."""
    if regime not in _FILES:
        rng = np.random.default_rng(REGIME_SEEDS[regime])
        out, lens = [], {}
        for sampling in S.SAMPLINGS:
            for h, w in SIZES:
                for dri in DRIS:
                    for tables in ('flat', 'skewed'):
                        hd = S.synth(rng, h, w, sampling, regime, orientation=1 + len(out) % 8)
                        out.append(((sampling, h, w, dri, tables), hd, dri, tables, S.encode(hd, dri, tables, lens if tables == 'skewed' else None)))
        _FILES[regime] = (out, lens)
    return _FILES[regime]


REGIME_SEEDS = dict(natural=11, dc_only=12, one_ac=13, zone_b=14, zone_c=15)


def prelimit(hd):
    """Every component's inverse-DCT output before the range-limit table, as one flat array."""
    return np.concatenate([R.plane(c, hd['q'], prelimit=True).ravel() for c in hd['comps']])


def test_the_matrix_is_whole():
    for regime in ('natural', 'zone_b', 'zone_c'):
        fs = files(regime)[0]
        assert len(fs) == 4 * len(SIZES) * len(DRIS) * 2 and len(set(k for k, *_ in fs)) == len(fs)
        if regime != 'zone_c':          # (legal zone C keeps 8-bit quantisers)
            assert any(max(int(q.max()) for q in hd['q'].values()) > 255 for _, hd, *_ in fs) and \
                any(max(int(q.max()) for q in hd['q'].values()) <= 255 for _, hd, *_ in fs)          # 16-bit and 8-bit DQT
        assert set(hd['orientation'] for _, hd, *_ in fs) == set(range(1, 9))


@pytest.mark.parametrize('regime', ['natural', 'zone_b', 'zone_c'])
def test_round_trip(regime):
    """R.coefficients(encode(hd)) gives back coefficients, tables, size, restart interval and orientation."""
    for key, hd, dri, tables, b in files(regime)[0]:
        got = R.coefficients(b)
        assert (got['W'], got['H'], got['dri'], got['orientation']) == (hd['W'], hd['H'], dri, hd['orientation']), key
        assert (got['hmax'], got['vmax']) == (hd['hmax'], hd['vmax']) and len(got['comps']) == len(hd['comps']), key
        for g, c in zip(got['comps'], hd['comps']):
            assert (g['h'], g['v'], g['tq'], g['td'], g['ta']) == (c['h'], c['v'], c['tq'], c['td'], c['ta']), key
            assert g['coef'].dtype == np.int16 and g['coef'].shape == c['coef'].shape and np.array_equal(g['coef'], c['coef']), key
            assert np.array_equal(got['q'][g['tq']], hd['q'][c['tq']]), key
        for k in set((0, c['td']) for c in hd['comps']) | set((1, c['ta']) for c in hd['comps']):
            assert got['ht'][k] == S.TABLES[tables][k], key


def test_long_codes_were_written():
    """The skewed tables have symbols at every length from 10 to 16, past the library's 9-bit lookahead, and the files of
    the matrix use every one of those lengths."""
    for k, (bits, _) in S.TABLES['skewed'].items():
        if k[0] == 1:
            assert all(bits[ln - 1] > 0 for ln in range(10, 17)), k
    assert all(max(ln for ln in range(1, 17) if bits[ln - 1]) <= 9 for bits, _ in S.TABLES['flat'].values())
    lens = {}
    for regime in ('natural', 'zone_b', 'zone_c'):
        for ln, n in files(regime)[1].items():
            lens[ln] = lens.get(ln, 0) + n
    print('Huffman code lengths written with the skewed tables:', sorted(lens.items()))
    assert all(lens.get(ln, 0) > 0 for ln in range(10, 17)), lens


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from ppyolo_hip import _lib
    return _lib.lib()


@pytest.mark.parametrize('regime', ['natural', 'zone_b', 'zone_c'])
def test_host_stage(L, regime):
    """ppy_jpeg_info and ppy_jpeg_entropy_decode of encode(hd) give hd: coefficients (transposed inside a block), quantisers
    in stored order, block counts and offsets."""
    from ppyolo_hip import _lib
    for key, hd, dri, tables, b in files(regime)[0]:
        info = _lib.JpegInfo()
        assert L.ppy_jpeg_info(b, len(b), ctypes.byref(info)) == 0 and info.status == 0 and info.reason == b'', key
        assert (info.width, info.height, info.components, info.orientation, info.restart_interval) == \
            (hd['W'], hd['H'], len(hd['comps']), hd['orientation'], dri), key
        assert (info.out_width, info.out_height) == ((hd['H'], hd['W']) if hd['orientation'] >= 5 else (hd['W'], hd['H'])), key
        total = sum(c['coef'].size * 2 for c in hd['comps'])
        assert info.coef_bytes == total, key
        coef = np.full(total // 2 + 8, 0x5a5a, np.int16)
        desc = _lib.JpegDesc()
        desc.coef_base = 4096
        reason = ctypes.create_string_buffer(64)
        assert L.ppy_jpeg_entropy_decode(b, len(b), coef.ctypes.data, total, ctypes.byref(desc), reason) == 0, (key, reason.value)
        assert np.all(coef[total // 2:] == 0x5a5a), key
        assert (desc.width, desc.height, desc.components, desc.orientation, desc.coef_bytes, desc.coef_base) == \
            (hd['W'], hd['H'], len(hd['comps']), hd['orientation'], total, 4096), key
        off = 0
        for c, comp in enumerate(hd['comps']):
            bh, bw = comp['coef'].shape[:2]
            assert (info.blocks_h[c], info.blocks_w[c], info.h_samp[c], info.v_samp[c]) == (bh, bw, comp['h'], comp['v']), key
            assert (desc.blocks_h[c], desc.blocks_w[c], desc.h_samp[c], desc.v_samp[c], desc.coef_offset[c]) == (bh, bw, comp['h'], comp['v'], off), key
            mine = coef[off:off + bh * bw * 64].reshape(bh, bw, 8, 8)
            assert np.array_equal(mine.transpose(0, 1, 3, 2).reshape(bh, bw, 64), comp['coef']), key
            assert np.array_equal(np.array(desc.quant[c]).reshape(8, 8).T.reshape(64), hd['q'][comp['tq']]), key
            off += bh * bw * 64


def test_one_ac_visits_every_position():
    rng = np.random.default_rng(5)
    hd = S.synth(rng, 40, 300, '444', 'one_ac')
    for c in hd['comps']:
        co = c['coef'].reshape(-1, 64)
        assert ((co[:, 1:] != 0).sum(1) <= 1).all()
        assert set(np.nonzero(co[:, 1:])[1] + 1) == set(range(1, 64))
        q = hd['q'][c['tq']].reshape(8, 8)
        assert (q != q.T).sum() >= 40                           # an asymmetric table: a transposed block decodes differently


@pytest.mark.parametrize('regime', ['natural', 'dc_only', 'one_ac'])
def test_zone_a_equals_pillow(regime):
    """Zone A, every inverse-DCT sample in [-512, 511] before the range-limit table (asserted on the inputs): the
    restatement equals Pillow as it comes, SIMD or not."""
    from PIL import Image  # noqa: F401         a plain import: without Pillow this pin fails, it does not skip
    fs = files(regime)[0]
    blocks = 0
    for key, hd, dri, tables, b in fs:
        pre = prelimit(hd)
        assert pre.min() >= -512 and pre.max() <= 511, key
        for c in hd['comps']:
            assert np.array_equal(R.plane(c, hd['q'], prelimit=True), R.plane(c, hd['q'], prelimit=True, wide=True)), key
        assert np.array_equal(R.reconstruct(hd), S.pillow_pixels(b)), key
        assert np.array_equal(R.reconstruct(hd, apply_orientation=False), S.pillow_pixels(S.encode(dict(hd, orientation=1), dri, tables))), key
        blocks += pre.size // 64
    print('zone A, %s: %d files, %d blocks, all equal to Pillow' % (regime, len(fs), blocks))


@pytest.fixture(scope='module')
def no_simd_child():
    """`python jpeg_synth.py zones` in a process of its own whose libjpeg-turbo runs its C code (JSIMD_FORCENONE=1 is read
    when the library first decodes): restatement against Pillow, blocks that differ per zone."""
    env = dict(os.environ, JSIMD_FORCENONE='1')
    r = subprocess.run([sys.executable, os.path.abspath(S.__file__), 'zones'], env=env, cwd=os.path.dirname(os.path.abspath(S.__file__)),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


def outside_blocks(hd):
    """bool [block rows, block columns] of a grey image: the block has a pre-limit sample outside [-512, 511]."""
    pre = R.plane(hd['comps'][0], hd['q'], prelimit=True)
    bh, bw = pre.shape[0] // 8, pre.shape[1] // 8
    pre = pre.reshape(bh, 8, bw, 8)
    return (pre.min((1, 3)) < -512) | (pre.max((1, 3)) > 511)


def test_zone_b_follows_the_c_table(no_simd_child):
    """Zone B, outside [-512, 511] with no int32 overflow: the restatement equals libjpeg-turbo's C code in every block, and
    whatever inverse DCT this host's Pillow runs, it differs from the restatement only in blocks that leave the range."""
    assert no_simd_child['zone_b']['differ'] == 0 and no_simd_child['zone_b']['blocks'] > 400, no_simd_child
    blocks = out = differ = 0
    for i, hd in enumerate(S.zone_inputs('zone_b', 41)):
        c = hd['comps'][0]
        assert (np.abs(c['coef'].astype(np.int64) * hd['q'][0]).sum(-1) <= S.S_MAX).all()
        assert np.array_equal(R.plane(c, hd['q'], prelimit=True), R.plane(c, hd['q'], prelimit=True, wide=True))
        outside = outside_blocks(hd)
        d = S.differing_blocks(R.reconstruct(hd), S.pillow_pixels(S.encode(hd, dri=(0, 3)[i % 2], tables=('flat', 'skewed')[i // 2 % 2])))
        assert d.shape == outside.shape and not (d & ~outside).any(), i
        blocks, out, differ = blocks + d.size, out + int(outside.sum()), differ + int(d.sum())
    print('zone B: %d blocks, %d leave [-512, 511], %d of those differ from the Pillow of this process' % (blocks, out, differ))
    assert out >= blocks // 2 and blocks - out >= blocks // 5           # both kinds are there


def test_zone_c_inputs_overflow_int32(no_simd_child):
    """Zone C, an int32 intermediate overflows: pinned to nothing but the restatement (libjpeg's C code computes in a 64-bit
    JLONG).  The test only shows that its inputs are in the zone; what Pillow gives there is printed, not asserted."""
    blocks = differ = 0
    for hd in S.zone_inputs('zone_c', 43) + [S.synth(np.random.default_rng(44), 40, 300, 'grey', 'zone_c', legal=False)]:
        c = hd['comps'][0]
        if np.abs(c['coef']).max() <= 1023:
            assert max(int(q.max()) for q in hd['q'].values()) <= 255           # legal baseline: a file can carry it
        a, b = R.plane(c, hd['q']), R.plane(c, hd['q'], wide=True)
        d = (a != b).reshape(a.shape[0] // 8, 8, a.shape[1] // 8, 8).any((1, 3))
        blocks, differ = blocks + d.size, differ + int(d.sum())
    print('zone C: int32 wrap-around differs from int64 in %d of %d blocks; without SIMD, Pillow differs from the restatement in %d of %d'
          % (differ, blocks, no_simd_child['zone_c']['differ'], no_simd_child['zone_c']['blocks']))
    assert differ >= 0.9 * blocks
