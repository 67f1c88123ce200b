"""The device entropy stage of the JPEG decoder without a GPU: the host pre-pass (ppy_jpeg_scan_prepare) against a short
restatement, and the host twin of the kernels (ppy_jpeg_entropy_twin -- the same decode step, state comparison and
slot-to-address map, run lane by lane) against the host stage ppy_jpeg_entropy_decode.  Array equality everywhere."""
import ctypes

import numpy as np
import pytest

import jpeg_entropy_util as U
import jpeg_fixtures as F
import jpeg_ref as R
import jpeg_synth as S

OK, UNSUPPORTED, CORRUPT = U.OK, U.UNSUPPORTED, U.CORRUPT
SIZES = sorted({U.SUBSEQ_MIN, U.SUBSEQ_MID, U.SUBSEQ_DEFAULT, U.SUBSEQ_MAX})          # the largest too: one lane per segment for most files


@pytest.fixture(scope='module')
def L():
    return U.lib()


_SYNTH = U.synth_cases()


def _restart_cases():
    """dri 0, 1, 3, 9 on 25 MCUs: 25 segments (the marker number wraps past D7 three times), 9, 3 and 1."""
    out = []
    for dri in (0, 1, 3, 9):
        for tables in ('flat', 'skewed'):
            rng = np.random.default_rng(100 + dri)
            out.append(('restart-dri%d-%s' % (dri, tables), S.encode(S.synth(rng, 40, 40, '444', 'natural'), dri=dri, tables=tables)))
    return out


_FILES = [(n, F.data(n)) for n in F.names()] + _SYNTH + _restart_cases()


def restate(b):
    """The segments of the entropy-coded data: split at the restart markers, stuffed zeros dropped."""
    hd = R.parse(b)
    hm, vm = max(c['h'] for c in hd['comps']), max(c['v'] for c in hd['comps'])
    if len(hd['comps']) == 1:
        hm = vm = 1
    mcus = -(-hd['W'] // (8 * hm)) * -(-hd['H'] // (8 * vm))
    dri = hd['dri']
    nseg = -(-mcus // dri) if dri else 1
    p, n, segs = hd['data'], len(b), []
    for s in range(nseg):
        out = bytearray()
        while p < n:
            if b[p] != 0xFF:
                out.append(b[p])
                p += 1
            elif p + 1 < n and b[p + 1] == 0:
                out.append(0xFF)
                p += 2
            else:
                break
        first = s * dri if dri else 0
        segs.append((bytes(out), first, min(dri, mcus - first) if dri else mcus))
        if s + 1 < nseg:
            while b[p:p + 2] == b'\xff\xff':
                p += 1
            assert b[p] == 0xFF and b[p + 1] == 0xD0 + (s & 7)
            p += 2
    return segs


@pytest.mark.parametrize('name,b', _FILES, ids=[n for n, _ in _FILES])
def test_prepass_equals_host_descriptor_and_restatement(L, name, b):
    rc, reason, desc, rec, seg_bound = U.prepass(L, b, coef_base=4096)
    assert rc == OK and reason == '' and desc.coef_base == 4096
    hrc, _, _, hdesc = U.host_stage(L, b)
    assert hrc == OK
    hdesc.coef_base = 4096
    assert bytes(desc) == bytes(hdesc)
    H, seg, data = U.record_parts(rec)
    want = restate(b)
    assert H.segments == len(want) <= seg_bound and H.restart_interval == R.parse(b)['dri']
    at = 0
    for (byte_off, bit_len, first, count), (body, wfirst, wcount) in zip(seg.tolist(), want):
        assert (byte_off, bit_len, first, count) == (at, 8 * len(body), wfirst, wcount)
        assert data[at:at + len(body)].tobytes() == body
        pad = -len(body) % 4
        assert not data[at + len(body):at + len(body) + pad].any()          # the pad reads as zero bits
        at += len(body) + pad
    assert at == H.data_bytes


def test_restart_cases_wrap_the_marker_number(L):
    segs = {n: U.record_parts(U.prepass(L, b)[3])[0].segments for n, b in _restart_cases()}
    assert sorted(set(segs.values())) == [1, 3, 9, 25]


@pytest.mark.parametrize('name,kind', F.refused())
def test_prepass_refusals_equal_info(L, name, kind):
    from ppyolo_hip import _lib
    b = F.data(name)
    info = _lib.JpegInfo()
    rc = L.ppy_jpeg_info(b, len(b), ctypes.byref(info))
    prc, reason, _, _, _ = U.prepass(L, b)
    assert (prc, reason) == (rc, info.reason.decode())
    assert (rc == UNSUPPORTED) == (kind == 'unsupported')
    if kind == 'corrupt':          # the header is whole, the pre-pass passes; the decode finds the end
        st, rs, _, _ = U.twin(L, [b], U.SUBSEQ_MIN)
        assert st[0] == CORRUPT and 'ends early' in L.ppy_jpeg_reason_string(int(rs[0])).decode()
        assert U.host_stage(L, b)[0] == CORRUPT


def test_prepass_finds_restart_marker_damage(L):
    b = F.data('c420_dri_65x33')
    k = b.index(b'\xff\xd1', R.parse(b)['data'])
    for m in (b[:k] + b'\xff\xd3' + b[k + 2:], b[:k] + b[k + 2:], b[:k + 1]):          # wrong number, missing, file ends in it
        rc, reason, _, _, _ = U.prepass(L, m)
        assert rc == CORRUPT and reason == 'restart marker expected'
        assert U.host_stage(L, m)[0] == CORRUPT
    fill = b[:k] + b'\xff\xff\xff' + b[k:]                                               # fill bytes before the marker
    assert U.prepass(L, fill)[0] == OK
    want = U.host_stage(L, b)[2]
    for m in (fill, b[:-2], b + b'trailing'):                                            # and a missing EOI, trailing bytes
        assert U.device_stage_class(L, m, U.SUBSEQ_MIN, want) == OK
    # a scan buffer that is too small is refused, not overrun
    from ppyolo_hip import _lib
    bound = L.ppy_jpeg_scan_bytes(b, len(b), None)
    rec = np.zeros(bound + 16, np.uint8)
    off = -rec.ctypes.data % 16
    assert L.ppy_jpeg_scan_prepare(b, len(b), rec.ctypes.data + off, bound - 16, None, ctypes.byref(_lib.JpegDesc()), None) == -3


@pytest.mark.parametrize('subseq', SIZES)
@pytest.mark.parametrize('name,b', _FILES, ids=[n for n, _ in _FILES])
def test_twin_equals_host_stage(L, name, b, subseq):
    rc, _, want, _ = U.host_stage(L, b)
    assert rc == OK
    st, rs, _, coefs = U.twin(L, [b], subseq)
    assert st[0] == OK and rs[0] == 0
    assert np.array_equal(coefs[0], want)


def test_twin_mixed_batch(L):
    """Every fixture in one call: the per-image offsets of plan, scan buffer and coefficients."""
    files = [F.data(n) for n in F.names()]
    st, _, _, coefs = U.twin(L, files, U.SUBSEQ_MIN)
    assert not st.any()
    for b, c in zip(files, coefs):
        assert np.array_equal(c, U.host_stage(L, b)[2])


def test_cross_workgroup_step_runs(L):
    """U.link_case(): 96 x 96, 4:4:4, 'natural' coefficients, 'flat' tables, no restart interval, seed 777 -- 4018 bytes, one
    segment of 408 subsequences of 8 bytes: two groups of 256 lanes.  Fixed-length codes do not self-synchronise, so the
    second group's first lane starts from a wrong assumption and only the link step repairs the group: its counter was
    152 (all 152 lanes of the second group) when this input was chosen.  Candidates measured on the CPU: 64 x 64 4:2:0
    flat gave 0 (1471 bytes: one group), 130 x 131 4:4:4 flat 641.  At the default size the file is one group and the
    counter must be 0."""
    b = U.link_case()
    rc, _, want, _ = U.host_stage(L, b)
    assert rc == OK
    st, _, fixed, coefs = U.twin(L, [b], U.SUBSEQ_MIN)
    assert st[0] == OK and np.array_equal(coefs[0], want)
    assert fixed[0] > 0
    st, _, fixed, coefs = U.twin(L, [b], U.SUBSEQ_DEFAULT)
    assert st[0] == OK and np.array_equal(coefs[0], want) and fixed[0] == 0


def _same_class(L, m, subseq):
    rc, _, coef, _ = U.host_stage(L, m)
    assert rc in (OK, UNSUPPORTED, CORRUPT)
    got = U.device_stage_class(L, m, subseq, coef)
    assert got == rc, (got, rc)
    return rc


@pytest.mark.parametrize('name,stride', U.PREFIX_SWEEPS)
def test_every_prefix_same_status_class(L, name, stride):
    """The prefix sweep of test_jpeg_host.py: (pre-pass, twin) and (ppy_jpeg_info, ppy_jpeg_entropy_decode) agree on the
    status class of every prefix, and on the coefficients where it is OK; at the smallest and the default subsequence size."""
    seen = {OK: 0, CORRUPT: 0}
    for m in U.prefixes(name, stride):
        for subseq in (U.SUBSEQ_MIN, U.SUBSEQ_DEFAULT):
            rc = _same_class(L, m, subseq)
        seen[rc] += 1
    assert seen[OK] >= 1 and seen[CORRUPT] > 10


def test_byte_flips_same_status_class(L):
    """Every byte of a small file replaced by 0x00 / 0xFF / its complement."""
    seen = set()
    for (i, v), m in U.flips():
        seen.add(_same_class(L, m, U.SUBSEQ_MIN))
    assert seen == {OK, UNSUPPORTED, CORRUPT}


def test_python_batch_layout_feeds_the_twin(L):
    """JpegDecoder(entropy='device').entropy_decode() without a GPU: its staging buffer [table | plan | records] planned as
    reconstruct() plans it, decoded by the twin in place of the kernels."""
    from ppyolo_hip import _lib
    from ppyolo_hip.jpeg import JpegDecoder
    from ppyolo_hip._lib import PPYoloHipError
    d = JpegDecoder(device='cpu', entropy='device', subseq_bytes=U.SUBSEQ_MID, threads=4)
    names = F.names()
    hb = d.entropy_decode([F.data(n) for n in names])
    assert hb.entropy == 'device' and hb.total_bytes == hb.table_bytes + hb.plan_bytes + hb.scan_bytes
    assert hb.total_bytes < sum(len(F.data(n)) for n in names) + 12000 * len(names)          # compressed bytes, not coefficients
    h_plan = hb.stage.data_ptr() + hb.table_bytes
    ws = ctypes.c_size_t()
    assert L.ppy_jpeg_entropy_plan(hb.n, hb.descs, h_plan + hb.plan_bytes, hb.scan_bytes, (ctypes.c_longlong * hb.n)(*hb.scan_off),
                                   d.subseq_bytes, h_plan, hb.plan_bytes, ctypes.byref(ws)) == OK
    coef = np.full(hb.coef_bytes // 2, 0x5a5a, np.int16)
    status = np.zeros(3 * hb.n, np.int32)
    work = np.zeros(ws.value // 8 + 2, np.int64)
    assert L.ppy_jpeg_entropy_twin(hb.n, h_plan, h_plan, h_plan + hb.plan_bytes, d.subseq_bytes, coef.ctypes.data, hb.coef_bytes,
                                   status.ctypes.data, work.ctypes.data + (-work.ctypes.data % 16), ws.value) == OK
    assert not status[:2 * hb.n].any()
    for i, n in enumerate(names):
        dsc = hb.descs[i]
        assert np.array_equal(coef[dsc.coef_base // 2:(dsc.coef_base + dsc.coef_bytes) // 2], U.host_stage(L, F.data(n))[2]), n
    d.release(hb)
    with pytest.raises(PPYoloHipError) as e:          # refusals name the item and give the buffer back, as in host mode
        d.entropy_decode([F.data(names[0]), F.data(F.refused()[0][0])])
    assert 'item 1' in str(e.value)
    dri = F.data('c420_dri_65x33')
    k = dri.index(b'\xff\xd1', R.parse(dri)['data'])
    for _ in range(3):
        with pytest.raises(PPYoloHipError) as e:
            d.entropy_decode([F.data(names[0]), F.data(names[1]), dri[:k] + b'\xff\xd3' + dri[k + 2:]])
        assert 'item 2: corrupt JPEG: restart marker expected (code -5)' in str(e.value)
    with pytest.raises(PPYoloHipError):
        JpegDecoder(device='cpu', entropy='device', subseq_bytes=24)
    with pytest.raises(PPYoloHipError):
        JpegDecoder(device='cpu', entropy='gpu')
