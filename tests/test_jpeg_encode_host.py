"""Host side of the JPEG encoder through the C ABI (no GPU): the header writer and the quantiser tables against the goldens,
the host twin of the bit-packer (ppy_jpeg_enc_scan_host) on the restatement's coefficients against the goldens' scan bytes,
the decoder's ppy_jpeg_entropy_decode on the produced files, refusals with guard regions, and coefficient sets no photograph
produces (tests/jpeg_synth.py) through the twin and back."""
import ctypes

import numpy as np
import pytest

import jpeg_enc_cases as C
import jpeg_enc_ref as E
import jpeg_enc_util as U
import jpeg_fixtures as F
import jpeg_ref as R
import jpeg_synth as S


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from ppyolo_hip import _lib
    return _lib.lib()


def sub(s):
    return s if s != 'grey' else '4:4:4'


def split(data):
    """A file -> (SOI .. SOS, scan bytes, EOI)."""
    i = R.parse(data)['data']
    return data[:i], data[i:-2], data[-2:]


@pytest.mark.parametrize('case', C.golden_cases(), ids=lambda c: c[0])
def test_header_twin_and_decoder(L, case):
    name, s, q, r = case
    img, want = C.golden_pixels(name), C.golden_bytes(name)
    head, body, eoi = split(want)
    comps = 1 if img.ndim == 2 else 3
    p = U.params(q, sub(s), r)
    rc, got, reason, intact, _ = U.header(L, p, img.shape[1], img.shape[0], comps)
    assert (rc, reason, intact) == (0, '', True) and got == head and eoi == b'\xff\xd9'
    assert len(head) == L.ppy_jpeg_enc_header_bytes(comps, r)
    hd = E.coefficients(img, q, sub(s), r)
    rc, descs, sizes, reason = U.layout(L, p, [(img.shape[0], img.shape[1], comps)])
    assert rc == 0 and reason == ''
    d = descs[0]
    for c, comp in enumerate(hd['comps']):
        assert (d.blocks_h[c], d.blocks_w[c]) == comp['coef'].shape[:2] and (d.h_samp[c], d.v_samp[c]) == (comp['h'], comp['v'])
    assert d.scan_capacity == L.ppy_jpeg_enc_scan_capacity(d.blocks, d.segments) == 416 * d.blocks + 4 * d.segments
    coef = U.stored(hd)
    assert coef.nbytes == d.coef_bytes == sizes.coef_bytes
    rc, scan, reason, intact = U.scan_host(L, d, coef)
    assert (rc, reason, intact) == (0, '', True)
    assert scan == body
    # the decoder's host stage reads the coefficients back from the file
    from ppyolo_hip import _lib
    back = np.zeros(coef.size, np.int16)
    desc = _lib.JpegDesc()
    data = got + scan + b'\xff\xd9'
    assert L.ppy_jpeg_entropy_decode(data, len(data), back.ctypes.data, back.nbytes, ctypes.byref(desc), None) == 0
    assert np.array_equal(back, coef)
    assert [desc.coef_offset[c] for c in range(comps)] == [d.coef_offset[c] for c in range(comps)]


@pytest.mark.parametrize('q', C.QUALITIES)
def test_quantiser_tables(L, q):
    a, b = (ctypes.c_ushort * 64)(), (ctypes.c_ushort * 64)()
    assert L.ppy_jpeg_enc_quant(q, a, b) == 0
    lum, chrom = E.quant_tables(q)
    assert list(a) == lum.tolist() and list(b) == chrom.tolist()


@pytest.mark.parametrize('name', [c[0] for c in C.COCO])
def test_coco_sized_fixture(L, name):
    (s, q, r), px = [c[1:] for c in C.COCO if c[0] == name][0], F.pixels(name)
    hd = E.coefficients(px, q, s, r)
    p = U.params(q, s, r)
    rc, descs, sizes, reason = U.layout(L, p, [px.shape])
    rc, scan, reason, intact = U.scan_host(L, descs[0], U.stored(hd))
    assert (rc, intact) == (0, True)
    assert C.matches_coco(name, U.header(L, p, px.shape[1], px.shape[0], 3)[1] + scan + b'\xff\xd9')


def test_bad_parameters_are_refused_and_write_nothing(L):
    for kw, code, word in ((dict(quality=0), U.BAD_ARG, 'quality'), (dict(quality=101), U.BAD_ARG, 'quality'),
                           (dict(restart_interval=-1), U.BAD_ARG, 'restart'), (dict(restart_interval=65536), U.BAD_ARG, 'restart'),
                           (dict(subsampling=(1, 2)), U.UNSUPPORTED, 'sampling'), (dict(subsampling=(4, 1)), U.UNSUPPORTED, 'sampling'),
                           (dict(subsampling=(2, 4)), U.UNSUPPORTED, 'sampling')):
        p = U.params(**kw)
        rc, got, reason, intact, untouched = U.header(L, p, 16, 16, 3, capacity=1024)
        assert rc == code and word in reason and untouched, kw
        rc, descs, sizes, reason = U.layout(L, p, [(16, 16, 3)])
        assert rc == code and word in reason, kw
    a = (ctypes.c_ushort * 64)()
    assert L.ppy_jpeg_enc_quant(0, a, a) == U.BAD_ARG and L.ppy_jpeg_enc_quant(101, a, a) == U.BAD_ARG and not any(a)
    p = U.params()
    for shape in ((0, 16, 3), (16, 0, 3), (65536, 16, 3), (16, 65536, 1), (16, 16, 2), (16, 16, 4)):
        rc, descs, sizes, reason = U.layout(L, p, [(8, 8, 3), shape])
        assert rc == U.BAD_ARG and reason.startswith('image 1'), shape
        assert U.header(L, p, shape[1], shape[0], shape[2], capacity=1024)[0] == U.BAD_ARG
    rc, descs, sizes, reason = U.layout(L, p, [(8, 8, 3)], srcs=[(0, 23)])            # a row pitch below the row's bytes
    assert rc == U.BAD_ARG and 'stride' in reason
    assert L.ppy_jpeg_enc_header_bytes(2, 0) == 0 and L.ppy_jpeg_enc_scan_capacity(0, 1) == 0 and L.ppy_jpeg_enc_scan_capacity(1, 0) == 0


def test_small_buffers_are_refused_and_not_overrun(L):
    img = C.image('noise', 33, 35, False)
    p = U.params(100, '4:2:0', 1)
    rc, descs, sizes, reason = U.layout(L, p, [img.shape])
    d = descs[0]
    coef = U.stored(E.coefficients(img, 100, '4:2:0', 1))
    for cap in (0, 1, d.scan_capacity - 1):
        rc, scan, reason, intact = U.scan_host(L, d, coef, capacity=cap)
        assert rc == U.WORKSPACE and 'capacity' in reason and intact and scan == b''
    need = L.ppy_jpeg_enc_header_bytes(3, 1)
    for cap in (0, need - 1):
        rc, got, reason, intact, untouched = U.header(L, p, 33, 35, 3, capacity=cap)
        assert rc == U.WORKSPACE and untouched
    rc, scan, reason, intact = U.scan_host(L, d, coef[:-1])                          # fewer coefficients than the descriptor says
    assert rc == U.BAD_ARG and intact
    d.blocks_w[0] += 1                                                               # a descriptor edited by hand sizes nothing
    rc, scan, reason, intact = U.scan_host(L, d, coef)
    assert rc == U.BAD_ARG and 'descriptor' in reason and intact


def test_values_without_a_baseline_code_are_refused(L):
    p = U.params(100, '4:4:4', 0)
    rc, descs, sizes, reason = U.layout(L, p, [(8, 16, 1)])
    coef = np.zeros(128, np.int16)
    coef[0], coef[64] = 1024, -1024                                                  # DC difference -2048: size 12
    rc, scan, reason, intact = U.scan_host(L, descs[0], coef)
    assert rc == U.BAD_ARG and 'DC' in reason and intact
    coef[:] = 0
    coef[9] = 1024                                                                   # an AC value of size 11
    rc, scan, reason, intact = U.scan_host(L, descs[0], coef)
    assert rc == U.BAD_ARG and 'AC' in reason and intact


SYNTH = [(sampling, regime, w, h, dri) for sampling in ('grey', '444', '422', '420')
         for regime, w, h, dri in (('natural', 33, 35, 0), ('one_ac', 65, 33, 3), ('dc_only', 17, 9, 1), ('zone_c', 40, 24, 2))]


def synth_hd(sampling, regime, w, h, dri):
    """jpeg_synth.synth in its legal regime, with the standard tables' ids: what a baseline file with OUR tables can carry."""
    rng = np.random.default_rng([7, S.REGIMES.index(regime), w, h, dri])
    hd = S.synth(rng, h, w, sampling, regime)
    hd['dri'] = dri
    return hd


@pytest.mark.parametrize('case', SYNTH, ids=lambda c: '%s_%s_%dx%d_r%d' % c)
def test_synthetic_coefficients_through_the_twin_and_back(L, case):
    """Runs and sizes photographs do not produce: every AC position alone (ZRL chains), full-range values, DC-only blocks."""
    hd = synth_hd(*case)
    s, shape = U.hd_params(hd)
    p = U.params(50, s, case[4])
    rc, descs, sizes, reason = U.layout(L, p, [shape])
    assert rc == 0
    coef = U.stored(hd)
    rc, scan, reason, intact = U.scan_host(L, descs[0], coef)
    assert (rc, reason, intact) == (0, '', True)
    assert scan == E.scan(hd)                                                        # the restatement's bit-packer
    data = U.header(L, p, shape[1], shape[0], shape[2])[1] + scan + b'\xff\xd9'
    back = R.coefficients(data)
    for a, b in zip(back['comps'], hd['comps']):
        assert np.array_equal(a['coef'], b['coef'])
