"""Numpy-only restatement of the baseline JPEG encoder of ppyolo_hip (csrc/jpeg_encode.hip), i.e. of libjpeg-turbo with its
default settings -- jpeg_set_defaults, jpeg_set_quality(q, TRUE), JDCT_ISLOW, the standard Huffman tables, a JFIF 1.01 header
-- which is what cv2.imwrite(path, img, [IMWRITE_JPEG_QUALITY, q]) runs and what Pillow's
Image.save(buf, 'JPEG', quality=q, subsampling=s, restart_marker_blocks=r) writes.

encode(img, quality, subsampling, restart_interval) -> (file bytes, hd, flags):
  img    uint8 [h,w,3] BGR (a YCbCr file) or [h,w] (a grey file);
  hd     the dict jpeg_ref.coefficients() returns for those bytes (W, H, comps with h, v, tq, td, ta, coef, q, dri, ...): the
         coefficient arrays are the seam between the two device stages, dummy blocks included;
  flags  which paths of the entropy coder and of the block grid the image took (FLAGS), so a test can assert its inputs
         reach them all.
header(), quant_tables(), scan() are the parts, for the tests that drive one stage alone.  Written for reading, not for speed;
tests/test_jpeg_enc_ref.py holds it equal to Pillow byte for byte (DESIGN.md section 10b names the steps)."""
import struct

import numpy as np

from jpeg_ref import ZZ

SUBSAMPLINGS = {'4:4:4': (1, 1), '4:2:2': (2, 1), '4:2:0': (2, 2)}
FLAGS = ('stuffed_ff', 'zrl', 'dc_size_11', 'ac_size_10', 'no_eob', 'dummy_right', 'dummy_below', 'dummy_both', 'rst_wrap')

# ISO/IEC 10918-1 Annex K.1, natural (row-major) order
Q_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51,
                   87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101,
                   72, 92, 95, 98, 112, 100, 103, 99])
Q_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99] +
                    [99] * 36)
# Annex K.3: (counts of the code lengths 1..16, symbols in code order) per (class, table id)
_AC_LUMA = [1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209,
            240, 36, 51, 98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70,
            71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121,
            122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167,
            168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212,
            213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248,
            249, 250]
_AC_CHROMA = [0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82,
              240, 21, 98, 114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68,
              69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119,
              120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164,
              165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202,
              210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247,
              248, 249, 250]
HUFF = {(0, 0): ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12))),
        (0, 1): ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12))),
        (1, 0): ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], _AC_LUMA),
        (1, 1): ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119], _AC_CHROMA)}


def _codes(spec):
    """symbol -> (code, length), the canonical assignment of Annex C."""
    out, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(spec[0][ln - 1]):
            out[spec[1][k]] = (code, ln)
            k += 1
            code += 1
        code <<= 1
    return out


CODES = {k: _codes(v) for k, v in HUFF.items()}


def quant_tables(quality):
    """jpeg_set_quality(q, force_baseline=TRUE): (luma, chroma), int32 [64] in natural order."""
    if not 1 <= quality <= 100:
        raise ValueError('quality %r' % (quality,))
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((t * scale + 50) // 100, 1, 255).astype(np.int32) for t in (Q_LUMA, Q_CHROMA))


def _seg(marker, payload):
    return b'\xff' + bytes([marker]) + struct.pack('>H', len(payload) + 2) + payload


def _layout(ncomp, subsampling):
    if ncomp == 1:
        return [dict(id=1, h=1, v=1, tq=0, td=0, ta=0)]
    h, v = SUBSAMPLINGS[subsampling]
    return [dict(id=1, h=h, v=v, tq=0, td=0, ta=0), dict(id=2, h=1, v=1, tq=1, td=1, ta=1), dict(id=3, h=1, v=1, tq=1, td=1, ta=1)]


def header(width, height, ncomp, quality=95, subsampling='4:2:0', restart_interval=0):
    """SOI, APP0, DQT (one per table), SOF0, DHT (DC then AC per table), [DRI], SOS: the order libjpeg's jcmarker.c writes."""
    comps = _layout(ncomp, subsampling)
    q = quant_tables(quality)
    out = [b'\xff\xd8', _seg(0xE0, b'JFIF\0\1\1\0\0\1\0\1\0\0')]
    for t in range(2 if ncomp == 3 else 1):
        out.append(_seg(0xDB, bytes([t]) + q[t][ZZ].astype(np.uint8).tobytes()))
    out.append(_seg(0xC0, struct.pack('>BHHB', 8, height, width, ncomp) + b''.join(bytes([c['id'], c['h'] << 4 | c['v'], c['tq']]) for c in comps)))
    for t in range(2 if ncomp == 3 else 1):
        for tc in (0, 1):
            out.append(_seg(0xC4, bytes([tc << 4 | t]) + bytes(HUFF[(tc, t)][0]) + bytes(HUFF[(tc, t)][1])))
    if restart_interval:
        out.append(_seg(0xDD, struct.pack('>H', restart_interval)))
    out.append(_seg(0xDA, bytes([ncomp]) + b''.join(bytes([c['id'], c['td'] << 4 | c['ta']]) for c in comps) + b'\0\x3f\0'))
    return b''.join(out)


# ------------------------------------------------------------------------------------------------------------- stage 1
def ycc(bgr):
    """jccolor.c rgb_ycc_convert: 16-bit fixed point; Y rounds with ONE_HALF, Cb and Cr carry (128 << 16) + ONE_HALF - 1."""
    b, g, r = (bgr[..., k].astype(np.int64) for k in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return [y, cb, cr]


def _pad(p, rows, cols):
    """Edge replication to [rows, cols]."""
    return np.pad(p, ((0, rows - p.shape[0]), (0, cols - p.shape[1])), mode='edge')


def component_plane(p, hs, vs, bw, bh):
    """One full-resolution component [H, W] -> its samples [bh * 8, bw * 8] (bw, bh = the REAL blocks, ceil(comp size / 8)),
    hs x vs = the full-resolution pixels under one sample.  To the right the FULL-RESOLUTION rows are extended by their last
    pixel (jcsample.c expand_right_edge) and the box filter runs over the extension, so a sample right of the image averages
    copies of the edge pixels.  Downwards the full-resolution rows are extended by the last row only up to a whole row group
    (vs rows, jcprepct.c); below that the last row of SAMPLES is repeated (expand_bottom_edge on the downsampled rows).  An
    8 x 8 image at 4:2:0 tells the two apart: rows 4..7 of its chroma block repeat sample row 3."""
    p = _pad(p, -(-p.shape[0] // vs) * vs, bw * 8 * hs)
    if (hs, vs) == (2, 1):
        bias = np.arange(p.shape[1] // 2) & 1                      # 0, 1, 0, 1, ...
        p = (p[:, 0::2] + p[:, 1::2] + bias) >> 1
    elif (hs, vs) == (2, 2):
        bias = 1 + (np.arange(p.shape[1] // 2) & 1)                # 1, 2, 1, 2, ...
        p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
    return _pad(p, bh * 8, bw * 8)


def fdct(s):
    """jfdctint.c jpeg_fdct_islow on level-shifted samples [..., 8, 8] -> coefficients scaled by 8."""
    def p(d, first):
        t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
        t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
        t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
        sh = 11 if first else 15                                   # CONST_BITS -+ PASS1_BITS
        r = 1 << (sh - 1)
        o = [None] * 8
        if first:
            o[0], o[4] = (t10 + t11) << 2, (t10 - t11) << 2
        else:
            o[0], o[4] = (t10 + t11 + 2) >> 2, (t10 - t11 + 2) >> 2
        z1 = (t12 + t13) * 4433
        o[2] = (z1 + t13 * 6270 + r) >> sh
        o[6] = (z1 - t12 * 15137 + r) >> sh
        z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
        z5 = (z3 + z4) * 9633
        t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
        z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
        o[7], o[5], o[3], o[1] = (t4 + z1 + z3 + r) >> sh, (t5 + z2 + z4 + r) >> sh, (t6 + z2 + z3 + r) >> sh, (t7 + z1 + z4 + r) >> sh
        return o

    s = s.astype(np.int64)
    ws = np.stack(p([s[..., :, k] for k in range(8)], True), axis=-1)              # pass 1: rows
    return np.stack(p([ws[..., r, :] for r in range(8)], False), axis=-2)          # pass 2: columns


def quantise(c, q):
    """jcdctmgr.c: divide by 8 * q, rounding half away from zero."""
    d = 8 * q.astype(np.int64)
    return np.sign(c) * ((np.abs(c) + (d >> 1)) // d)


def coefficients(img, quality=95, subsampling='4:2:0', restart_interval=0):
    """Stage 1: pixels -> the dict jpeg_ref.coefficients() returns, plus hd['dummy'] = set of 'right' / 'below' / 'both'."""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] != 3):
        raise ValueError('uint8 [h,w,3] or [h,w] expected')
    H, W = img.shape[:2]
    planes = ycc(img) if img.ndim == 3 else [img.astype(np.int64)]
    comps = _layout(len(planes), subsampling)
    hm, vm = comps[0]['h'], comps[0]['v']
    mx, my = -(-W // (8 * hm)), -(-H // (8 * vm))
    qt = quant_tables(quality)
    dummy = set()
    for c, p in zip(comps, planes):
        hs, vs = hm // c['h'], vm // c['v']
        bw, bh = -(-(-(-W // hs)) // 8), -(-(-(-H // vs)) // 8)        # real blocks: ceil(ceil(W / hs) / 8)
        s = component_plane(p, hs, vs, bw, bh) - 128
        blk = s.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)
        co = quantise(fdct(blk), qt[c['tq']].reshape(8, 8)).reshape(bh, bw, 64)
        full = np.zeros((my * c['v'], mx * c['h'], 64), np.int64)
        full[:bh, :bw] = co
        # dummy blocks (jccoefct.c compress_data): AC zero, DC = the DC of the block before them in the MCU's block order
        for y in range(full.shape[0]):
            for x in range(full.shape[1]):
                if y < bh and x < bw:
                    continue
                dummy.add('both' if y >= bh and x >= bw else 'below' if y >= bh else 'right')
                py, px = (y, x - 1) if x % c['h'] else (y - 1, x + c['h'] - 1)      # previous block of the same MCU
                full[y, x, 0] = full[py, px, 0]
        c['coef'] = full.astype(np.int16)
    return dict(W=W, H=H, comps=comps, q={0: qt[0], 1: qt[1]}, dri=restart_interval, orientation=1, hmax=hm, vmax=vm, dummy=dummy)


# ------------------------------------------------------------------------------------------------------------- stage 2
def scan(hd, flags=None):
    """jchuff.c: the entropy-coded bytes of hd's coefficients, stuffed, with the RSTn markers; no EOI."""
    comps, dri = hd['comps'], hd['dri']
    mx, my = -(-hd['W'] // (8 * hd['hmax'])), -(-hd['H'] // (8 * hd['vmax']))
    zz = ZZ.tolist()
    blocks = [c['coef'].astype(np.int64)[:, :, zz] for c in comps]
    nz = [[[np.flatnonzero(row[1:]).tolist() for row in line] for line in b] for b in blocks]
    blocks = [b.tolist() for b in blocks]
    fl = set()
    out, acc, nbits, pred = [], 0, 0, [0] * len(comps)

    def flush():
        nonlocal acc, nbits
        pad = -nbits % 8
        acc, nbits = acc << pad | (1 << pad) - 1, nbits + pad      # the last byte is filled with 1-bits
        raw = acc.to_bytes(nbits // 8, 'big')
        if b'\xff' in raw:
            fl.add('stuffed_ff')
        out.append(raw.replace(b'\xff', b'\xff\0'))
        acc = nbits = 0

    for m in range(mx * my):
        y, x = divmod(m, mx)
        if dri and m and m % dri == 0:
            flush()
            k = m // dri - 1
            if k >= 8:
                fl.add('rst_wrap')
            out.append(bytes([0xFF, 0xD0 + (k & 7)]))
            pred = [0] * len(comps)
        for ci, c in enumerate(comps):
            dc, ac = CODES[(0, c['td'])], CODES[(1, c['ta'])]
            for v in range(c['v']):
                for h in range(c['h']):
                    by, bx = y * c['v'] + v, x * c['h'] + h
                    b = blocks[ci][by][bx]
                    d = b[0] - pred[ci]
                    pred[ci] = b[0]
                    s = abs(d).bit_length()
                    if s == 11:
                        fl.add('dc_size_11')
                    code, ln = dc[s]
                    acc, nbits = (acc << ln | code) << s | ((d if d >= 0 else d - 1) & (1 << s) - 1), nbits + ln + s
                    last = 0
                    for k in nz[ci][by][bx]:
                        k += 1
                        run = k - last - 1
                        while run > 15:
                            fl.add('zrl')
                            code, ln = ac[0xF0]
                            acc, nbits = acc << ln | code, nbits + ln
                            run -= 16
                        a = b[k]
                        s = abs(a).bit_length()
                        if s == 10:
                            fl.add('ac_size_10')
                        code, ln = ac[run << 4 | s]
                        acc, nbits = (acc << ln | code) << s | ((a if a >= 0 else a - 1) & (1 << s) - 1), nbits + ln + s
                        last = k
                    if last < 63:
                        code, ln = ac[0]
                        acc, nbits = acc << ln | code, nbits + ln
                    else:
                        fl.add('no_eob')
    flush()
    if flags is not None:
        flags |= fl
    return b''.join(out)


def encode(img, quality=95, subsampling='4:2:0', restart_interval=0):
    """-> (file bytes, hd, flags)."""
    img = np.asarray(img)
    hd = coefficients(img, quality, subsampling, restart_interval)
    flags = set('dummy_' + d for d in hd['dummy'])
    body = scan(hd, flags)
    data = header(hd['W'], hd['H'], len(hd['comps']), quality, subsampling, restart_interval) + body + b'\xff\xd9'
    return data, hd, flags
