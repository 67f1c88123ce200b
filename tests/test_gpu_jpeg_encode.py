"""The JPEG encoder on the device (csrc/jpeg_encode.hip) against its two CPU definitions: stage 1 against the numpy
restatement (tests/jpeg_enc_ref.py), element for element, dummy blocks included; device stage 2 against the host twin
(ppy_jpeg_enc_scan_host), byte for byte and length for length; JpegEncoder.encode against the stored libjpeg-turbo bytes
(tests/golden/g21_jpeg_encode.npz).  Equality everywhere; no Pillow, nothing outside the repository.

Tile edges of the kernels, as (width, height) of GREY images, whose blocks are their MCUs (8 pixels of width = one block):
  stage 1, 32 blocks per workgroup ................................ 31, 32, 33 blocks: (248, 8), (256, 8), (257, 8)
  bit-packer, 64 blocks per workgroup ............................. 63, 64, 65 blocks: (504, 8), (512, 8), (513, 8)
  prefix sums, 1024 blocks / restart segments per round ........... 1023, 1024, 1025: (8184, 8), (8192, 8), (8193, 8), the
                                                                    segments at restart interval 1
  0xFF counts, 1024 chunks of 64 unstuffed bytes per round ........ a (512, 320) noise image at quality 100, whose stream is
                                                                    asserted to exceed two rounds (131072 bytes)"""
import ctypes

import numpy as np
import pytest
import torch

import jpeg_enc_cases as C
import jpeg_enc_ref as E
import jpeg_enc_util as U
import jpeg_fixtures as F
import jpeg_ref as R
import jpeg_synth as S

pytestmark = pytest.mark.gpu

TILE_EDGES = ((248, 8), (256, 8), (257, 8), (504, 8), (512, 8), (513, 8), (8184, 8), (8192, 8), (8193, 8))
MIXED = (('noise', 33, 35, False), ('smooth', 65, 33, True), ('noise', 1, 1, False), ('checker', 40, 24, False), ('flat', 17, 9, True))


def sub(s):
    return s if s != 'grey' else '4:4:4'


def encoder(**kw):
    from ppyolo_hip.jpeg import JpegEncoder
    return JpegEncoder(**kw)


_REF = {}


def ref(img, q, s, r):
    """The restatement's (file, hd) of an image, computed once per process."""
    key = (img.shape, img.tobytes(), q, s, r)
    if key not in _REF:
        data, hd, _ = E.encode(img, q, s, r)
        _REF[key] = (data, hd)
    return _REF[key]


def check_stage1(enc, images, sources=None):
    """enc.coefficients(sources or images) == the restatement of `images`, per component and block; -> the EncBatch."""
    eb = enc.coefficients(images if sources is None else sources)
    flat = eb.coef.cpu().numpy()
    for i, img in enumerate(images):
        d = eb.descs[i]
        hd = ref(img, enc.quality, enc.subsampling, enc.restart_interval)[1]
        got = U.natural(d, flat[d.coef_base:d.coef_base + d.coef_bytes].view(np.int16))
        assert len(got) == len(hd['comps'])
        for c, (g, comp) in enumerate(zip(got, hd['comps'])):
            assert g.shape == comp['coef'].shape and np.array_equal(g, comp['coef']), \
                (i, img.shape, c, np.argwhere(g != comp['coef'])[:4].tolist())
    return eb


def check_stage2(enc, eb):
    """Device stage 2 == host twin on the coefficient buffer of eb: lengths and bytes; -> the scans."""
    out, lengths = enc.scan_device(eb)
    lens = lengths.cpu().tolist()
    twin = enc.scan_host(eb)
    assert lens == [len(t) for t in twin]
    data = out[:sum(lens)].cpu().numpy().tobytes()
    assert data == b''.join(twin)
    return twin


def batch_of(enc, hds):
    """An EncBatch whose coefficient buffer holds the given coefficient dicts (stage 2 never reads the pixels)."""
    from ppyolo_hip import _lib
    from ppyolo_hip.jpeg import EncBatch
    L = _lib.lib()
    pixel = torch.zeros(16, dtype=torch.uint8, device='cuda')
    n = len(hds)
    rc, descs, sizes, reason = U.layout(L, enc.params, [U.hd_params(hd)[1] for hd in hds],
                                        srcs=[(pixel.data_ptr(), 3 * 65535)] * n)
    assert rc == 0, reason
    host = np.zeros(sizes.coef_bytes // 2, np.int16)
    for d, hd in zip(descs, hds):
        assert U.hd_params(hd)[0] == enc.subsampling or len(hd['comps']) == 1
        st = U.stored(hd)
        assert st.nbytes == d.coef_bytes
        host[d.coef_base // 2:d.coef_base // 2 + st.size] = st
    table = np.zeros(sizes.table_bytes, np.uint8)
    assert L.ppy_jpeg_enc_pack_table(ctypes.byref(enc.params), n, descs, table.ctypes.data, sizes.table_bytes) == 0
    eb = EncBatch()
    eb.n, eb.descs, eb.sizes, eb.sources = n, descs, sizes, [pixel]
    eb.table, eb.coef = torch.from_numpy(table).cuda(), torch.from_numpy(host.view(np.uint8)).cuda()
    return eb


# ---- a + b on the same buffers ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('restart', C.RESTARTS)
@pytest.mark.parametrize('sampling', C.SAMPLINGS)
def test_all_sizes_in_one_batch(sampling, restart):
    """Every size of the grid in one call, contents and a quality per (sampling, restart) in turn."""
    k = C.SAMPLINGS.index(sampling) * 3 + C.RESTARTS.index(restart)
    q = C.QUALITIES[k % len(C.QUALITIES)]
    images = [C.image(C.CONTENTS[(k + i) % 4], w, h, sampling == 'grey') for i, (w, h) in enumerate(C.SIZES)]
    enc = encoder(quality=q, subsampling=sub(sampling), restart_interval=restart)
    eb = check_stage1(enc, images)
    twin = check_stage2(enc, eb)
    for img, t in zip(images, twin):            # and the twin's bytes are the restatement's
        data = ref(img, q, sub(sampling), restart)[0]
        assert data[R.parse(data)['data']:-2] == t


@pytest.mark.parametrize('restart', (0, 1))
def test_tile_edges(restart):
    images = [C.image('noise' if i % 2 else 'smooth', w, h, True) for i, (w, h) in enumerate(TILE_EDGES)]
    enc = encoder(quality=90, restart_interval=restart)
    eb = check_stage1(enc, images)
    assert [int(d.blocks) for d in eb.descs] == [31, 32, 33, 63, 64, 65, 1023, 1024, 1025]
    assert restart == 0 or [int(d.segments) for d in eb.descs][-3:] == [1023, 1024, 1025]
    check_stage2(enc, eb)


def test_long_stream_crosses_the_chunk_rounds():
    img = C.image('noise', 512, 320, True)
    enc = encoder(quality=100, restart_interval=3)               # (one setting: the restatement of this image takes seconds)
    eb = check_stage1(enc, [img])
    twin = check_stage2(enc, eb)
    assert len(twin[0]) > 2 * 1024 * 64 and twin[0].count(b'\xff\x00') > 100


@pytest.mark.parametrize('sampling', ('4:4:4', '4:2:2', '4:2:0'))
def test_mixed_batch_strided_view_and_decoder_output(sampling):
    """Five images of mixed sizes, grey ones among them, one of them a view into a larger tensor read in place, plus the
    output of JpegDecoder used as it comes."""
    from ppyolo_hip.jpeg import JpegDecoder
    images = [C.image(c, w, h, g) for c, w, h, g in MIXED]
    big = torch.from_numpy(C.image('noise', 80, 60, False)).cuda()
    sources = [torch.from_numpy(a).cuda() for a in images]
    h, w = images[0].shape[:2]
    big[3:3 + h, 5:5 + w] = sources[0]
    sources[0] = big[3:3 + h, 5:5 + w]
    assert not sources[0].is_contiguous() and sources[0].data_ptr() != big.data_ptr()
    bigg = torch.from_numpy(C.image('noise', 90, 50, True)).cuda()
    h, w = images[1].shape
    bigg[2:2 + h, 7:7 + w] = sources[1]
    sources[1] = bigg[2:2 + h, 7:7 + w]
    decoded = JpegDecoder().decode([F.data('c420_37x53')])[0]
    images.append(F.pixels('c420_37x53'))
    sources.append(decoded)
    for restart in (0, 3):
        enc = encoder(quality=75, subsampling=sampling, restart_interval=restart)
        eb = check_stage1(enc, images, sources)
        check_stage2(enc, eb)
    assert np.array_equal(big[3:3 + 35, 5:5 + 33].cpu().numpy(), images[0])         # the sources are read, never written


SYNTH = [(regime, w, h) for regime, w, h in (('natural', 33, 35), ('one_ac', 65, 33), ('dc_only', 17, 9), ('zone_c', 40, 24), ('one_ac', 520, 24))]


@pytest.mark.parametrize('restart', C.RESTARTS)
@pytest.mark.parametrize('sampling', ('grey', '444', '422', '420'))
def test_synthetic_coefficients(sampling, restart):
    """Coefficient sets photographs do not produce (tests/jpeg_synth.py, legal regime): every AC position alone, values over
    the whole baseline range, DC-only blocks."""
    hds = []
    for regime, w, h in SYNTH:
        hd = S.synth(np.random.default_rng([11, S.REGIMES.index(regime), w, h]), h, w, sampling, regime)
        hd['dri'] = restart
        hds.append(hd)
    enc = encoder(quality=50, subsampling={'grey': '4:4:4', '444': '4:4:4', '422': '4:2:2', '420': '4:2:0'}[sampling], restart_interval=restart)
    twin = check_stage2(enc, batch_of(enc, hds))
    for hd, t in zip(hds, twin):
        assert t == E.scan(hd)


# ---- c ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('entropy', ('device', 'host'))
def test_encode_equals_the_goldens(entropy):
    from ppyolo_hip.jpeg import JpegDecoder
    dec = JpegDecoder()
    for name, s, q, r in C.golden_cases():
        img, want = C.golden_pixels(name), C.golden_bytes(name)
        enc = encoder(quality=q, subsampling=sub(s), restart_interval=r, entropy=entropy)
        got = enc.imencode(torch.from_numpy(img).cuda())
        assert got == want, name
        assert enc.imencode(img) == want, name                                      # numpy inputs are uploaded
        if entropy == 'device':
            assert np.array_equal(dec.decode([got])[0].cpu().numpy(), R.decode(want)), name


@pytest.mark.parametrize('entropy', ('device', 'host'))
def test_coco_sized_fixtures(entropy):
    names = [c[0] for c in C.COCO]
    enc = encoder(entropy=entropy)                                                  # the defaults: 95, 4:2:0, no restarts
    got = enc.encode([torch.from_numpy(F.pixels(n)).cuda() for n in names])
    for n, data in zip(names, got):
        assert C.matches_coco(n, data), n


def test_imwrite(tmp_path):
    name, s, q, r = C.golden_cases()[-1]
    path = str(tmp_path / 'out.jpg')
    encoder(quality=q, subsampling=sub(s), restart_interval=r).imwrite(path, torch.from_numpy(C.golden_pixels(name)).cuda())
    assert open(path, 'rb').read() == C.golden_bytes(name)


# ---- d ------------------------------------------------------------------------------------------------------------------
def test_reuse_does_not_depend_on_stale_buffers():
    large, small = C.image('noise', 512, 320, False), C.image('smooth', 33, 35, False)
    kw = dict(quality=100, subsampling='4:2:0', restart_interval=3)
    used = encoder(**kw)
    first = used.imencode(large)
    after = used.imencode(small)
    assert after == encoder(**kw).imencode(small) == ref(small, 100, '4:2:0', 3)[0]
    assert used.imencode(large) == first and used.encode([small, large]) == [after, first]
    assert first == ref(large, 100, '4:2:0', 3)[0]


# ---- e ------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from ppyolo_hip._lib import PPYoloHipError
    for kw, word in ((dict(quality=0), 'quality'), (dict(quality=101), 'quality'), (dict(quality=50.0), 'quality'),
                     (dict(subsampling='4:1:1'), 'subsampling'), (dict(subsampling=(2, 2)), 'subsampling'),
                     (dict(restart_interval=-1), 'restart_interval'), (dict(restart_interval=65536), 'restart_interval'),
                     (dict(entropy='auto'), 'entropy')):
        with pytest.raises(PPYoloHipError, match=word):
            encoder(**kw)
    enc = encoder()
    ok = torch.zeros((16, 24, 3), dtype=torch.uint8, device='cuda')
    bad = ((ok.float(), 'dtype'), (ok.to(torch.int8), 'dtype'), (ok[None], 'shape'), (ok[:, :, :2], 'shape'), (ok[:, :, 0][:, :, None], 'shape'),
           (ok[:, ::2], 'strides'), (ok.permute(1, 0, 2), 'strides'), (ok[::2, ::3], 'strides'),
           (ok[:, :, 0], 'strides'), (ok[:1].expand(4, 24, 3), 'strides'), (torch.zeros((0, 4, 3), dtype=torch.uint8, device='cuda'), '1..65535'),
           (torch.zeros((1, 65536), dtype=torch.uint8, device='cuda'), '1..65535'), (np.zeros((4, 4, 3), np.float32), 'dtype'),
           (np.zeros((4, 4, 4), np.uint8), 'shape'), ([[1, 2], [3, 4]], 'expected a uint8 tensor'), (b'bytes', 'expected a uint8 tensor'))
    for im, word in bad:
        with pytest.raises(PPYoloHipError, match=word):
            enc.encode([ok, im])
    with pytest.raises(PPYoloHipError, match='empty'):
        enc.encode([])
    if torch.cuda.device_count() > 1:
        with pytest.raises(PPYoloHipError, match='lives on'):
            enc.encode([ok.to('cuda:1')])
    assert enc.encode([ok])[0] == enc.encode([ok.cpu()])[0] == enc.encode([ok.cpu().numpy()])[0]      # and the encoder still works


def test_small_device_buffers_are_refused_on_the_host():
    from ppyolo_hip import _lib
    L = _lib.lib()
    enc = encoder()
    eb = enc.coefficients([C.image('smooth', 33, 35, False)])
    s = eb.sizes
    ws = torch.empty(s.ws_bytes, dtype=torch.uint8, device='cuda')
    out = torch.full((s.out_bytes,), 0xA5, dtype=torch.uint8, device='cuda')
    lengths = torch.full((1,), -7, dtype=torch.int64, device='cuda')
    stream = torch.cuda.current_stream().cuda_stream

    def call(out_bytes=s.out_bytes, ws_bytes=s.ws_bytes, coef_bytes=s.coef_bytes):
        return L.ppy_jpeg_enc_scan_device(1, eb.descs, eb.table.data_ptr(), eb.coef.data_ptr(), coef_bytes, out.data_ptr(), out_bytes,
                                          lengths.data_ptr(), ws.data_ptr(), ws_bytes, stream)
    assert call(out_bytes=s.out_bytes - 1) == U.WORKSPACE and call(ws_bytes=s.ws_bytes - 1) == U.WORKSPACE
    assert call(coef_bytes=s.coef_bytes - 1) == U.BAD_ARG
    assert L.ppy_jpeg_enc_coefficients(1, eb.descs, eb.table.data_ptr(), eb.coef.data_ptr(), s.coef_bytes - 1, stream) == U.BAD_ARG
    torch.cuda.synchronize()
    assert int(lengths[0]) == -7 and bool((out == 0xA5).all())                     # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert 0 < int(lengths[0]) <= s.out_bytes
