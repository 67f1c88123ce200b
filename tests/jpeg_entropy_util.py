"""The device entropy stage of the JPEG decoder through the C ABI, for the tests on both sides of it: the host pre-pass
(ppy_jpeg_scan_prepare), the batch plan, the host twin of the kernels (ppy_jpeg_entropy_twin) and the host stage they must
equal (ppy_jpeg_entropy_decode); the seeded synthetic files; and the damaged streams of the sweeps."""
import ctypes

import numpy as np

import jpeg_fixtures as F
import jpeg_synth as S

OK, UNSUPPORTED, CORRUPT = 0, -2, -5
SUBSEQ_MIN, SUBSEQ_MID, SUBSEQ_DEFAULT, SUBSEQ_MAX = 8, 16, 32, 4096
BIG = 1 << 27          # a damaged header may claim gigabytes of coefficients: such a file is judged by its header alone (no single-byte
                       # change of the swept files comes near: the largest claims 65321 x 41 pixels, 21 MB)


def lib():
    import __graft_entry__ as ge
    ge.build()
    from ppyolo_hip import _lib
    assert (SUBSEQ_MIN, SUBSEQ_DEFAULT, SUBSEQ_MAX) == (_lib.JPEG_SUBSEQ_MIN, _lib.JPEG_SUBSEQ_DEFAULT, _lib.JPEG_SUBSEQ_MAX)
    return _lib.lib()


def host_stage(L, b):
    """(ppy_jpeg_info, then ppy_jpeg_entropy_decode) -> (status, reason, coefficients or None, descriptor)."""
    from ppyolo_hip import _lib
    info = _lib.JpegInfo()
    rc = L.ppy_jpeg_info(b, len(b), ctypes.byref(info))
    if rc != OK or info.coef_bytes > BIG:
        return rc, info.reason.decode(), None, None
    coef = np.full(max(info.coef_bytes // 2, 1), 0x5a5a, np.int16)
    desc = _lib.JpegDesc()
    reason = ctypes.create_string_buffer(64)
    rc = L.ppy_jpeg_entropy_decode(b, len(b), coef.ctypes.data, info.coef_bytes, ctypes.byref(desc), reason)
    return rc, reason.value.decode(), (coef if rc == OK else None), desc


def _aligned(nbytes, fill=0xA5):
    raw = np.full(nbytes + 16, fill, np.uint8)
    off = -raw.ctypes.data % 16
    return raw[off:off + nbytes]


def prepass(L, b, coef_base=0):
    """ppy_jpeg_scan_prepare -> (status, reason, descriptor, record as uint8 array of exactly its size, segment bound)."""
    from ppyolo_hip import _lib
    segs = ctypes.c_longlong()
    bound = L.ppy_jpeg_scan_bytes(b, len(b), ctypes.byref(segs))
    rec = _aligned(max(bound, 16))
    desc = _lib.JpegDesc()
    desc.coef_base = coef_base
    used = ctypes.c_size_t()
    reason = ctypes.create_string_buffer(64)
    rc = L.ppy_jpeg_scan_prepare(b, len(b), rec.ctypes.data, bound, ctypes.byref(used), ctypes.byref(desc), reason)
    if rc == OK:
        assert 0 < used.value <= bound and used.value % 16 == 0
    return rc, reason.value.decode(), desc, rec[:used.value].copy(), segs.value


def record_parts(rec):
    """A scan record -> (header, segment table [segments, 4] uint32, data bytes)."""
    from ppyolo_hip import _lib
    H = _lib.JpegScan.from_buffer_copy(rec[:ctypes.sizeof(_lib.JpegScan)].tobytes())
    assert H.record_bytes == rec.size
    seg = rec[H.segment_offset:H.segment_offset + 16 * H.segments].view(np.uint32).reshape(H.segments, 4)
    return H, seg, rec[H.data_offset:H.data_offset + H.data_bytes]


class Batch(object):
    """Files that passed the pre-pass, laid out as ppyolo_hip/jpeg.py lays a batch out: [plan | records], coefficient offsets."""

    def __init__(self, L, files, subseq):
        from ppyolo_hip import _lib
        self.n = n = len(files)
        self.descs = (_lib.JpegDesc * n)()
        recs, offs, at, coef_at, segs = [], [], 0, 0, 0
        for i, b in enumerate(files):
            rc, reason, desc, rec, _ = prepass(L, b, coef_at)
            assert rc == OK, (i, rc, reason)
            self.descs[i] = desc
            coef_at += (desc.coef_bytes + 15) // 16 * 16
            recs.append(rec)
            offs.append(at)
            at += rec.size
            segs += record_parts(rec)[0].segments
        self.coef_bytes = coef_at
        self.scan = _aligned(at)
        self.scan[:] = np.concatenate(recs)
        self.scan_off = (ctypes.c_longlong * n)(*offs)
        self.plan_bytes = L.ppy_jpeg_entropy_plan_bytes(n, segs)
        self.plan = _aligned(self.plan_bytes)
        ws = ctypes.c_size_t()
        rc = L.ppy_jpeg_entropy_plan(n, self.descs, self.scan.ctypes.data, self.scan.size, self.scan_off, subseq, self.plan.ctypes.data,
                                     self.plan_bytes, ctypes.byref(ws))
        assert rc == OK, rc
        self.ws_bytes, self.subseq = ws.value, subseq

    def coefficients(self, coef, i):
        d = self.descs[i]
        return coef[d.coef_base // 2:(d.coef_base + d.coef_bytes) // 2]


def twin(L, files, subseq):
    """Pre-pass + plan + ppy_jpeg_entropy_twin -> (status [n], reason ids [n], fixed-by-the-link-step counters [n], coefficients)."""
    bt = Batch(L, files, subseq)
    coef = _aligned(bt.coef_bytes, 0x5A).view(np.int16)          # the call zeroes what it owns
    status = np.full(3 * bt.n, 77, np.int32)
    ws = _aligned(max(bt.ws_bytes, 16))
    rc = L.ppy_jpeg_entropy_twin(bt.n, bt.plan.ctypes.data, bt.plan.ctypes.data, bt.scan.ctypes.data, subseq, coef.ctypes.data, bt.coef_bytes,
                                 status.ctypes.data, ws.ctypes.data, bt.ws_bytes)
    assert rc == OK, rc
    n = bt.n
    return status[:n], status[n:2 * n], status[2 * n:], [bt.coefficients(coef, i) for i in range(n)]


def device_stage_class(L, b, subseq, want=None):
    """Status class of (pre-pass, then twin) for one file; where it is OK and `want` is given, the coefficients must equal it."""
    rc, _, desc, _, _ = prepass(L, b)
    if rc != OK or desc.coef_bytes > BIG:
        return rc
    st, _, _, coefs = twin(L, [b], subseq)
    if st[0] == OK and want is not None:
        assert np.array_equal(coefs[0], want)
    return int(st[0])


# ------------------------------------------------------------------------------------------------ seeded synthetic files
SYNTH_SIZES = [(1, 1), (8, 8), (9, 17), (33, 35), (64, 48), (130, 131)]


def synth_cases():
    """[(id, bytes)]: every sampling x regime x table set, the sizes in turn, restart intervals 0 / 1 / 3 / 9 in turn."""
    out = []
    k = 0
    for samp in ('grey', '444', '422', '420'):
        for regime in ('natural', 'dc_only', 'one_ac', 'zone_c'):
            for tables in ('flat', 'skewed'):
                h, w = SYNTH_SIZES[k % len(SYNTH_SIZES)]
                dri = (0, 1, 3, 9)[(k // 2) % 4]
                rng = np.random.default_rng(9000 + k)
                out.append(('%s-%s-%s-%dx%d-dri%d' % (samp, regime, tables, h, w, dri),
                            S.encode(S.synth(rng, h, w, samp, regime), dri=dri, tables=tables)))
                k += 1
    # the extremes of the size range in every sampling, whatever the rotation above gave them
    for i, samp in enumerate(('grey', '444', '422', '420')):
        for (h, w), regime, tables in (((1, 1), 'natural', 'skewed'), ((130, 131), 'zone_c', 'skewed'), ((130, 131), 'natural', 'flat')):
            rng = np.random.default_rng(9500 + 10 * i + h)
            out.append(('%s-%s-%s-%dx%d-dri0' % (samp, regime, tables, h, w), S.encode(S.synth(rng, h, w, samp, regime), dri=0, tables=tables)))
    return out


def link_case():
    """The input of the cross-workgroup test: a 'flat'-table file (fixed-length codes never self-synchronise) whose single
    segment spans several groups of 256 subsequences at the smallest subsequence size."""
    rng = np.random.default_rng(777)
    return S.encode(S.synth(rng, 96, 96, '444', 'natural'), dri=0, tables='flat')


# ------------------------------------------------------------------------------------------------------ damaged streams
PREFIX_SWEEPS = [('c420_dri_65x33', 1), ('c444_q16big_20x27', 1), ('segments_33x35', 1), ('coco_398725', 97)]
FLIP_FILE = 'c422_dri_opt_41x70'


def prefixes(name, stride):
    b = F.data(name)
    return [bytes(b[:n]) for n in list(range(0, len(b), stride)) + [len(b)]]


def flips(name=FLIP_FILE):
    b = F.data(name)
    return [((i, v), b[:i] + bytes([v]) + b[i + 1:]) for i in range(len(b)) for v in (0, 0xFF, b[i] ^ 0xFF)]
