"""Numpy-only restatement of the baseline JPEG decoder of ppyolo_hip (csrc/jpeg.hip), i.e. of libjpeg-turbo with its default
settings: JDCT_ISLOW inverse DCT (jidctint.c), fancy upsampling (jdsample.c), integer YCbCr tables (jdcolor.c), and the EXIF
orientation as cv2.imread applies it.  decode(bytes) -> uint8 [h,w,3] BGR = reconstruct(coefficients(bytes)): the
coefficient dict is the seam between the host stage and the device stage of the library, and the tests drive either side of
it.  Written for reading, not for speed; the test files compare it with Pillow (libjpeg-turbo) where Pillow exists and with
the library everywhere.

All inverse-DCT arithmetic is int32 with wrap-around, as in the kernel, and the result goes through libjpeg's C range-limit
table.  That equals every libjpeg-turbo build while a block's inverse DCT stays in [-512, 511] before the table (all encoder
output does); beyond it libjpeg-turbo's SIMD code saturates where the C table wraps, and once an int32 intermediate
overflows libjpeg's 64-bit JLONG differs too (tests/test_jpeg_synth.py)."""
import struct

import numpy as np

ZZ = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
               28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
               54, 47, 55, 62, 63])


class JpegUnsupported(ValueError):
    """A valid file outside the subset (PPY_ERR_UNSUPPORTED)."""


class JpegCorrupt(ValueError):
    """Not a JPEG, or damaged / truncated (PPY_ERR_CORRUPT)."""


def exif_orientation(s):
    """Orientation (1..8) from the payload of an APP1 segment; 1 when it holds none."""
    if s[:6] != b'Exif\0\0' or len(s) < 14:
        return 1
    t = s[6:]
    e = {b'II': '<', b'MM': '>'}.get(bytes(t[:2]))
    if e is None or struct.unpack(e + 'H', t[2:4])[0] != 42:
        return 1
    off = struct.unpack(e + 'I', t[4:8])[0]
    if off + 2 > len(t):
        return 1
    for k in range(struct.unpack(e + 'H', t[off:off + 2])[0]):
        p = off + 2 + 12 * k
        if p + 12 > len(t):
            return 1
        tag, typ, cnt = struct.unpack(e + 'HHI', t[p:p + 8])
        if tag == 0x0112:
            v = struct.unpack(e + 'H', t[p + 8:p + 10])[0]
            return v if typ == 3 and cnt == 1 and 1 <= v <= 8 else 1
    return 1


def parse(b):
    """Markers up to and including SOS -> dict(W, H, comps, q, ht, dri, orientation, data = offset of the entropy data)."""
    b = bytes(b)
    if b[:2] != b'\xff\xd8':
        raise JpegCorrupt('no SOI')
    i = 2
    q, ht, dri, sof, orient, jfif, adobe = {}, {}, 0, None, None, False, None
    while True:
        if i + 2 > len(b) or b[i] != 0xFF:
            raise JpegCorrupt('marker expected')
        m = b[i + 1]
        i += 2
        if m == 0xFF:                           # fill byte
            i -= 1
            continue
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m == 0xD9 or m == 0xD8 or m == 0:
            raise JpegCorrupt('unexpected marker %02x' % m)
        if i + 2 > len(b):
            raise JpegCorrupt('truncated')
        L = struct.unpack('>H', b[i:i + 2])[0]
        if L < 2 or i + L > len(b):
            raise JpegCorrupt('truncated segment')
        s = b[i + 2:i + L]
        i += L
        if m == 0xDB:
            j = 0
            while j < len(s):
                pq, tq = s[j] >> 4, s[j] & 15
                j += 1
                if pq > 1 or tq > 3 or j + 64 * (pq + 1) > len(s):
                    raise JpegCorrupt('DQT')
                t = np.frombuffer(s[j:j + 64 * (pq + 1)], '>u2' if pq else 'u1').astype(np.int32)
                j += 64 * (pq + 1)
                q[tq] = np.zeros(64, np.int32)
                q[tq][ZZ] = t
        elif m in (0xC0, 0xC1):
            if sof is not None or len(s) < 6:
                raise JpegCorrupt('SOF')
            p, H, W, n = struct.unpack('>BHHB', s[:6])
            if len(s) < 6 + 3 * n:
                raise JpegCorrupt('SOF')
            if p != 8:
                raise JpegUnsupported('%d-bit samples' % p)
            if H == 0 or W == 0:
                raise JpegUnsupported('zero size')
            if n not in (1, 3):
                raise JpegUnsupported('%d components' % n)
            sof = dict(H=H, W=W, comps=[dict(id=s[6 + 3 * k], h=s[7 + 3 * k] >> 4, v=s[7 + 3 * k] & 15, tq=s[8 + 3 * k])
                                        for k in range(n)])
        elif m in (0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF):
            raise JpegUnsupported('progressive' if m == 0xC2 else 'arithmetic' if m >= 0xC9 else 'SOF%d' % (m - 0xC0))
        elif m == 0xCC:
            raise JpegUnsupported('arithmetic')
        elif m == 0xC4:
            j = 0
            while j < len(s):
                if j + 17 > len(s):
                    raise JpegCorrupt('DHT')
                tc, th = s[j] >> 4, s[j] & 15
                cnt = list(s[j + 1:j + 17])
                j += 17
                if tc > 1 or th > 3 or sum(cnt) > 256 or j + sum(cnt) > len(s):
                    raise JpegCorrupt('DHT')
                ht[(tc, th)] = (cnt, list(s[j:j + sum(cnt)]))
                j += sum(cnt)
        elif m == 0xDD:
            if len(s) < 2:
                raise JpegCorrupt('DRI')
            dri = struct.unpack('>H', s[:2])[0]
        elif m == 0xE0 and s[:5] == b'JFIF\0':
            jfif = True
        elif m == 0xE1 and orient is None and s[:6] == b'Exif\0\0':
            orient = exif_orientation(s)
        elif m == 0xEE and s[:5] == b'Adobe' and len(s) >= 12:
            adobe = s[11]
        elif m == 0xDA:
            if sof is None:
                raise JpegCorrupt('SOS before SOF')
            comps = sof['comps']
            if len(s) < 1 or len(s) < 4 + 2 * s[0]:
                raise JpegCorrupt('SOS')
            if s[0] != len(comps):
                raise JpegUnsupported('multiple scans')
            for k, c in enumerate(comps):
                if s[1 + 2 * k] != c['id']:
                    raise JpegUnsupported('scan component order')
                c['td'], c['ta'] = s[2 + 2 * k] >> 4, s[2 + 2 * k] & 15
            if len(comps) == 3:
                if adobe == 0 or (adobe is None and not jfif and [c['id'] for c in comps] == [82, 71, 66]):
                    raise JpegUnsupported('RGB (Adobe transform 0)')
                if (comps[1]['h'], comps[1]['v'], comps[2]['h'], comps[2]['v']) != (1, 1, 1, 1) or \
                        (comps[0]['h'], comps[0]['v']) not in ((1, 1), (2, 1), (2, 2)):
                    raise JpegUnsupported('sampling factors')
            else:
                if not (1 <= comps[0]['h'] <= 4 and 1 <= comps[0]['v'] <= 4):
                    raise JpegCorrupt('sampling factors')
                comps[0]['h'] = comps[0]['v'] = 1           # a one-component scan is never interleaved
            for c in comps:
                if c['tq'] not in q or (0, c['td']) not in ht or (1, c['ta']) not in ht:
                    raise JpegCorrupt('missing table')
            return dict(W=sof['W'], H=sof['H'], comps=comps, q=q, ht=ht, dri=dri, orientation=orient or 1, data=i)


_LUTS = {}


def _lut(spec):
    """16-bit peek -> (code length, symbol); length 0 = no such code."""
    key = (tuple(spec[0]), tuple(spec[1]))
    if key not in _LUTS:
        _LUTS[key] = _build_lut(spec)
    return _LUTS[key]


def _build_lut(spec):
    cnt, syms = spec
    ln_ = np.zeros(65536, np.int64)
    sy_ = np.zeros(65536, np.int64)
    code = k = 0
    for ln in range(1, 17):
        for _ in range(cnt[ln - 1]):
            if code >= (1 << ln):
                raise JpegCorrupt('bad Huffman table')
            lo = code << (16 - ln)
            ln_[lo:lo + (1 << (16 - ln))] = ln
            sy_[lo:lo + (1 << (16 - ln))] = syms[k]
            k += 1
            code += 1
        code <<= 1
    return ln_.tolist(), sy_.tolist()


class _Bits(object):
    """Bit reader over the entropy data: byte-unstuffs up to the next marker, and refuses to read past it."""

    def __init__(self, b, p):
        self.b, self.p = b, p
        self.load()

    def load(self):
        b, p = self.b, self.p
        out = bytearray()
        while True:
            j = b.find(b'\xff', p)
            if j < 0 or j + 1 >= len(b):
                out += b[p:] if j < 0 else b[p:j]
                p = len(b)
                break
            out += b[p:j]
            if b[j + 1] == 0:
                out.append(0xFF)
                p = j + 2
            else:
                p = j
                break
        self.p = p                              # at the marker (or the end of the file)
        self.n = 8 * len(out)
        self.seg = bytes(out) + b'\0\0\0\0'
        self.pos = 0

    def peek16(self):
        w = int.from_bytes(self.seg[self.pos >> 3:(self.pos >> 3) + 4], 'big')
        return (w >> (16 - (self.pos & 7))) & 0xFFFF

    def skip(self, k):
        self.pos += k
        if self.pos > self.n:
            raise JpegCorrupt('entropy data ends early')

    def sym(self, lut):
        w = self.peek16()
        if lut[0][w] == 0:
            raise JpegCorrupt('bad Huffman code')
        self.skip(lut[0][w])
        return lut[1][w]

    def bits(self, k):
        if k == 0:
            return 0
        v = self.peek16() >> (16 - k)
        self.skip(k)
        return v

    def restart(self, k):
        b, p = self.b, self.p
        while p + 1 < len(b) and b[p] == 0xFF and b[p + 1] == 0xFF:
            p += 1
        if p + 1 >= len(b) or b[p] != 0xFF or b[p + 1] != 0xD0 + (k & 7):
            raise JpegCorrupt('restart marker expected')
        self.p = p + 2
        self.load()


def _ext(v, t):
    return v if t == 0 or v >= (1 << (t - 1)) else v - (1 << t) + 1


def coefficients(b):
    """parse(b) + c['coef'] per component: int16 [block rows, block columns, 64] in natural (row-major) order, not
    dequantised.  Block counts are those of whole MCUs."""
    b = bytes(b)
    hd = parse(b)
    comps = hd['comps']
    hm, vm = max(c['h'] for c in comps), max(c['v'] for c in comps)
    mx, my = -(-hd['W'] // (8 * hm)), -(-hd['H'] // (8 * vm))
    for c in comps:
        c['coef'] = np.zeros((my * c['v'], mx * c['h'], 64), np.int16)
        c['dc'], c['ac'] = _lut(hd['ht'][(0, c['td'])]), _lut(hd['ht'][(1, c['ta'])])
    br = _Bits(b, hd['data'])
    pred = [0] * len(comps)
    cnt = 0
    zz = ZZ.tolist()
    for y in range(my):
        for x in range(mx):
            if hd['dri'] and cnt and cnt % hd['dri'] == 0:
                br.restart(cnt // hd['dri'] - 1)
                pred = [0] * len(comps)
            cnt += 1
            for ci, c in enumerate(comps):
                for v in range(c['v']):
                    for h in range(c['h']):
                        blk = [0] * 64
                        t = br.sym(c['dc'])
                        if t > 15:
                            raise JpegCorrupt('bad DC size')
                        pred[ci] += _ext(br.bits(t), t)
                        blk[0] = pred[ci]
                        k = 1
                        while k < 64:
                            rs = br.sym(c['ac'])
                            r, s_ = rs >> 4, rs & 15
                            if s_ == 0:
                                if r != 15:
                                    break
                                k += 16
                                continue
                            k += r
                            if k > 63:
                                raise JpegCorrupt('coefficient index past 63')
                            blk[zz[k]] = _ext(br.bits(s_), s_)
                            k += 1
                        c['coef'][y * c['v'] + v, x * c['h'] + h] = np.array(blk, np.int64).astype(np.int16)
    hd['hmax'], hd['vmax'] = hm, vm
    return hd


def idct(c, prelimit=False, wide=False):
    """jidctint.c jpeg_idct_islow on dequantised blocks [..., 8, 8] -> samples 0..255, or with prelimit=True the values that
    index the range-limit table (the sample less 128).  wide=True evaluates in int64, where nothing can overflow (libjpeg's
    JLONG on a 64-bit host), instead of int32 with wrap-around."""
    np_int = np.int64 if wide else np.int32
    c = c.astype(np_int)

    def p(i0, i1, i2, i3, i4, i5, i6, i7, sh):
        z1 = (i2 + i6) * np_int(4433)
        t2 = z1 + i6 * np_int(-15137)
        t3 = z1 + i2 * np_int(6270)
        t0 = (i0 + i4) << 13
        t1 = (i0 - i4) << 13
        t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
        a0, a1, a2, a3 = i7, i5, i3, i1
        z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
        z5 = (z3 + z4) * np_int(9633)
        a0, a1, a2, a3 = a0 * np_int(2446), a1 * np_int(16819), a2 * np_int(25172), a3 * np_int(12299)
        z1, z2 = z1 * np_int(-7373), z2 * np_int(-20995)
        z3, z4 = z3 * np_int(-16069) + z5, z4 * np_int(-3196) + z5
        a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
        r = np_int(1 << (sh - 1))
        return [(v + r) >> sh for v in (t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3)]

    with np.errstate(over='ignore'):
        ws = np.stack(p(*[c[..., r, :] for r in range(8)], 11), axis=-2)            # pass 1: columns
        out = np.stack(p(*[ws[..., :, k] for k in range(8)], 18), axis=-1)          # pass 2: rows
    if prelimit:
        return out
    # the range-limit TABLE of jdmaster.c, centred on 128 and indexed & 1023: it wraps, it does not clamp
    tab = np.concatenate([np.arange(128, 256), np.full(384, 255), np.zeros(384, int), np.arange(0, 128)])
    return tab[out & 1023]


def plane(c, q, prelimit=False, wide=False):
    """One component as a block-padded plane [block rows * 8, block columns * 8]; prelimit / wide as in idct."""
    np_int = np.int64 if wide else np.int32
    co = (c['coef'].astype(np_int) * q[c['tq']].astype(np_int)).reshape(c['coef'].shape[0], c['coef'].shape[1], 8, 8)
    px = idct(co, prelimit, wide)
    return px.transpose(0, 2, 1, 3).reshape(px.shape[0] * 8, px.shape[1] * 8)


def h2v1(p, n):
    p = p[:, :n].astype(np.int64)
    o = np.zeros((p.shape[0], 2 * n), np.int64)
    L = np.concatenate([p[:, :1], p[:, :-1]], 1)
    R = np.concatenate([p[:, 1:], p[:, -1:]], 1)
    o[:, 0::2] = (3 * p + L + 1) >> 2
    o[:, 1::2] = (3 * p + R + 2) >> 2
    o[:, 0] = p[:, 0]
    o[:, -1] = p[:, -1]
    return o


def h2v2(p, n, m):
    p = p[:m, :n].astype(np.int64)
    up = np.concatenate([p[:1], p[:-1]])
    dn = np.concatenate([p[1:], p[-1:]])
    o = np.zeros((2 * m, 2 * n), np.int64)
    for v, nb in ((0, up), (1, dn)):
        t = 3 * p + nb
        L = np.concatenate([t[:, :1], t[:, :-1]], 1)
        R = np.concatenate([t[:, 1:], t[:, -1:]], 1)
        e = (3 * t + L + 8) >> 4
        od = (3 * t + R + 7) >> 4
        e[:, 0] = (4 * t[:, 0] + 8) >> 4
        od[:, -1] = (4 * t[:, -1] + 7) >> 4
        o[v::2, 0::2] = e
        o[v::2, 1::2] = od
    return o


def orient(a, o):
    """EXIF orientation o applied to an [h,w,c] array (what ImageOps.exif_transpose / cv2.imread do)."""
    if o == 2:
        a = a[:, ::-1]
    elif o == 3:
        a = a[::-1, ::-1]
    elif o == 4:
        a = a[::-1]
    elif o == 5:
        a = a.transpose(1, 0, 2)
    elif o == 6:
        a = np.rot90(a, -1)
    elif o == 7:
        a = a[::-1, ::-1].transpose(1, 0, 2)
    elif o == 8:
        a = np.rot90(a, 1)
    return np.ascontiguousarray(a)


def reconstruct(hd, apply_orientation=True):
    """The device stage: coefficients -> pixels.  hd as coefficients() returns it; only W, H, orientation, q and the
    components' h, v, tq, coef are read."""
    H, W = hd['H'], hd['W']
    hm, vm = max(c['h'] for c in hd['comps']), max(c['v'] for c in hd['comps'])
    pl = []
    for c in hd['comps']:
        p = plane(c, hd['q'])
        dw, dh = -(-W * c['h'] // hm), -(-H * c['v'] // vm)
        if c['h'] == hm and c['v'] == vm:
            o = p
        elif dw <= 2:                                   # jdsample.c: fancy upsampling needs more than 2 columns
            o = np.repeat(np.repeat(p, hm // c['h'], 1), vm // c['v'], 0)
        elif c['v'] == vm:
            o = h2v1(p, dw)
        else:
            o = h2v2(p, dw, dh)
        pl.append(o[:H, :W].astype(np.int64))
    if len(pl) == 1:
        out = np.stack([pl[0]] * 3, -1).astype(np.uint8)
    else:
        y, cb, cr = pl
        x = np.arange(256) - 128
        crr = (91881 * x + 32768) >> 16
        cbb = (116130 * x + 32768) >> 16
        crg = -46802 * x
        cbg = -22554 * x + 32768
        r = np.clip(y + crr[cr], 0, 255)
        g = np.clip(y + ((cbg[cb] + crg[cr]) >> 16), 0, 255)
        bl = np.clip(y + cbb[cb], 0, 255)
        out = np.stack([bl, g, r], -1).astype(np.uint8)
    return orient(out, hd['orientation']) if apply_orientation else out


def decode(b, apply_orientation=True):
    return reconstruct(coefficients(b), apply_orientation)
