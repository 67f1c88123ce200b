"""Numpy restatement of what JpegDecoder(accept=...) adds to the baseline decoder restated in tests/jpeg_ref.py: the scan loop
(several scans per frame, tables that change between them), progressive coefficient decoding as libjpeg's jdphuff.c does it,
the completeness rule, and the two further upsamplers of jdsample.c.  It builds on jpeg_ref (bit reader, Huffman tables,
inverse DCT, planes, orientation) and returns the same coefficient dict, so jpeg_ref's users can read it.

coefficients(bytes, accept) -> dict; reconstruct(dict) -> uint8 [h,w,3] BGR; decode = the two in turn.  accept is the mask of
include/ppyolo_hip.h: PROGRESSIVE | MULTISCAN | SAMPLING; with 0 this refuses what jpeg_ref.parse refuses."""
import struct

import numpy as np

import jpeg_ref as R
from jpeg_ref import JpegCorrupt, JpegUnsupported

PROGRESSIVE, MULTISCAN, SAMPLING = 1, 2, 4
ALL = 7
MAX_SCANS = 256


def _tables(m, s, st):
    """DQT / DHT / DRI / APPn and the refused frame types: one segment (marker m, payload s) into the state dict st."""
    if m == 0xDB:
        j = 0
        while j < len(s):
            pq, tq = s[j] >> 4, s[j] & 15
            j += 1
            if pq > 1 or tq > 3 or j + 64 * (pq + 1) > len(s):
                raise JpegCorrupt('DQT')
            t = np.frombuffer(s[j:j + 64 * (pq + 1)], '>u2' if pq else 'u1').astype(np.int32)
            j += 64 * (pq + 1)
            st['q'][tq] = np.zeros(64, np.int32)
            st['q'][tq][R.ZZ] = t
    elif 0xC9 <= m <= 0xCF:
        raise JpegUnsupported('arithmetic')
    elif m in (0xC3, 0xC5, 0xC6, 0xC7):
        raise JpegUnsupported('lossless or hierarchical')
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
            st['ht'][(tc, th)] = R._lut((cnt, list(s[j:j + sum(cnt)])))
            j += sum(cnt)
    elif m == 0xDD:
        if len(s) < 2:
            raise JpegCorrupt('DRI')
        st['dri'] = struct.unpack('>H', s[:2])[0]
    elif m == 0xE0 and s[:5] == b'JFIF\0':
        st['jfif'] = True
    elif m == 0xE1 and st['orient'] is None and s[:6] == b'Exif\0\0':
        st['orient'] = R.exif_orientation(s)
    elif m == 0xEE and s[:5] == b'Adobe' and len(s) >= 12:
        st['adobe'] = s[11]


def _frame_checks(st, accept):
    comps = st['comps']
    if len(comps) == 3:
        if st['adobe'] == 0 or (st['adobe'] is None and not st['jfif'] and [c['id'] for c in comps] == [82, 71, 66]):
            raise JpegUnsupported('RGB (Adobe transform 0)')
        h, v = comps[0]['h'], comps[0]['v']
        chroma = (comps[1]['h'], comps[1]['v'], comps[2]['h'], comps[2]['v']) == (1, 1, 1, 1)
        if not accept & SAMPLING:
            if not chroma or (h, v) not in ((1, 1), (2, 1), (2, 2)):
                raise JpegUnsupported('sampling factors')
        else:
            if not (1 <= h <= 4 and 1 <= v <= 4):
                raise JpegCorrupt('sampling factors')
            if not chroma:
                raise JpegUnsupported('chroma sampling factors')
            if h * v > 8:
                raise JpegUnsupported('more than 10 blocks in an MCU')
    else:
        if not (1 <= comps[0]['h'] <= 4 and 1 <= comps[0]['v'] <= 4):
            raise JpegCorrupt('sampling factors')
        comps[0]['h'] = comps[0]['v'] = 1
    hm, vm = comps[0]['h'], comps[0]['v']
    st['hmax'], st['vmax'] = hm, vm
    st['mx'], st['my'] = -(-st['W'] // (8 * hm)), -(-st['H'] // (8 * vm))
    for c in comps:
        c['coef'] = np.zeros((st['my'] * c['v'], st['mx'] * c['h'], 64), np.int64)      # natural order; int16 at the end
        c['bits'] = [-1] * 64                                                          # libjpeg's coef_bits: -1 = never sent
        c['q'] = None                                                                  # latched at the component's first scan


def _scan_header(s, st, accept):
    comps, prog = st['comps'], st['progressive']
    if len(s) < 1 or len(s) < 4 + 2 * s[0]:
        raise JpegCorrupt('SOS')
    ns = s[0]
    if not prog and not accept & MULTISCAN:
        if ns != len(comps):
            raise JpegUnsupported('multiple scans')
        if [s[1 + 2 * k] for k in range(ns)] != [c['id'] for c in comps]:
            raise JpegUnsupported('scan component order')
    if not 1 <= ns <= len(comps):
        raise JpegCorrupt('SOS')
    sc, ids = [], [c['id'] for c in comps]
    for k in range(ns):
        if s[1 + 2 * k] not in ids:
            raise JpegCorrupt('unknown component')
        ci = ids.index(s[1 + 2 * k])
        if ci in [e[0] for e in sc]:
            raise JpegCorrupt('component twice')
        sc.append((ci, s[2 + 2 * k] >> 4, s[2 + 2 * k] & 15))
    if ns > 1 and sum(comps[ci]['h'] * comps[ci]['v'] for ci, _, _ in sc) > 10:
        raise JpegCorrupt('more than 10 blocks in an MCU')
    ss, se, ah, al = s[1 + 2 * ns], s[2 + 2 * ns], s[3 + 2 * ns] >> 4, s[3 + 2 * ns] & 15
    need_dc = need_ac = True
    if prog:
        if ss > 63 or se > 63 or se < ss or ah > 13 or al > 13:
            raise JpegCorrupt('scan parameters out of range')
        if ss == 0 and se != 0:
            raise JpegCorrupt('DC scan with Se != 0')
        if ss != 0 and ns != 1:
            raise JpegCorrupt('AC scan with more than one component')
        if ah != 0 and ah != al + 1:
            raise JpegCorrupt('refinement with Ah != Al + 1')
        need_dc, need_ac = ss == 0 and ah == 0, ss != 0
    else:
        ss, se, ah, al = 0, 63, 0, 0
    for ci, td, ta in sc:
        c = comps[ci]
        if c['q'] is None and c['tq'] not in st['q']:
            raise JpegCorrupt('missing table')
        if (need_dc and (0, td) not in st['ht']) or (need_ac and (1, ta) not in st['ht']):
            raise JpegCorrupt('missing table')
        for j in range(ss, se + 1):
            if not prog and c['bits'][j] >= 0:
                raise JpegCorrupt('scan repeats a component')
            if prog and ah != max(c['bits'][j], 0):
                raise JpegCorrupt('scan out of progression order')
    return sc, ss, se, ah, al


def _eob_run(br, r):
    return (1 << r) + (br.bits(r) if r else 0)


def _block(br, kind, blk, dc, ac, pred, ss, se, al, eobrun):
    """One block (a list of 64 ints, natural order, updated in place) of a scan -> (pred, eobrun)."""
    zz = _ZZ
    if kind == 'seq':
        t = br.sym(dc)
        if t > 15:
            raise JpegCorrupt('bad DC size')
        pred += R._ext(br.bits(t), t)
        blk[0] = pred
        k = 1
        while k < 64:
            rs = br.sym(ac)
            r, s = rs >> 4, rs & 15
            if s == 0:
                if r != 15:
                    break
                k += 16
                continue
            k += r
            if k > 63:
                raise JpegCorrupt('coefficient index past 63')
            blk[zz[k]] = R._ext(br.bits(s), s)
            k += 1
    elif kind == 'dc_first':
        t = br.sym(dc)
        if t > 15:
            raise JpegCorrupt('bad DC size')
        pred += R._ext(br.bits(t), t)
        blk[0] = pred * (1 << al)
    elif kind == 'dc_refine':
        if br.bits(1):
            blk[0] |= 1 << al
    elif kind == 'ac_first':
        if eobrun > 0:
            return pred, eobrun - 1
        k = ss
        while k <= se:
            rs = br.sym(ac)
            r, s = rs >> 4, rs & 15
            if s:
                k += r
                if k > se:
                    raise JpegCorrupt('coefficient index past the end of the band')
                blk[zz[k]] = R._ext(br.bits(s), s) * (1 << al)
            elif r == 15:
                k += 15
            else:
                eobrun = _eob_run(br, r) - 1
                break
            k += 1
    else:                                                           # ac_refine
        p1 = 1 << al

        def correct(pos):
            if br.bits(1) and (blk[pos] & p1) == 0:               # Python's & on a negative int is two's complement, as in C
                blk[pos] += p1 if blk[pos] >= 0 else -p1

        k = ss
        if eobrun == 0:
            while k <= se:
                rs = br.sym(ac)
                r, s = rs >> 4, rs & 15
                val = 0
                if s:
                    if s != 1:
                        raise JpegCorrupt('bad value in a refinement scan')
                    val = p1 if br.bits(1) else -p1
                elif r != 15:
                    eobrun = _eob_run(br, r)
                    break
                while k <= se:
                    if blk[zz[k]] != 0:
                        correct(zz[k])
                    else:
                        r -= 1
                        if r < 0:
                            break
                    k += 1
                if val:
                    if k > se:
                        raise JpegCorrupt('coefficient index past the end of the band')
                    blk[zz[k]] = val
                k += 1
        if eobrun > 0:
            while k <= se:
                if blk[zz[k]] != 0:
                    correct(zz[k])
                k += 1
            eobrun -= 1
    return pred, eobrun


_ZZ = R.ZZ.tolist()


def _run_scan(b, pos, st, scan):
    sc, ss, se, ah, al = scan
    comps = st['comps']
    inter = len(sc) > 1
    if inter:
        ux, uy = st['mx'], st['my']
    else:                                   # one component: the blocks that hold image samples, not the MCU padding
        c = comps[sc[0][0]]
        ux = -(-(-(-st['W'] * c['h'] // st['hmax'])) // 8)
        uy = -(-(-(-st['H'] * c['v'] // st['vmax'])) // 8)
    kind = 'seq' if not st['progressive'] else ('dc_refine' if ah else 'dc_first') if ss == 0 else ('ac_refine' if ah else 'ac_first')
    br = R._Bits(b, pos)
    pred, eobrun, unit, dri = [0] * len(sc), 0, 0, st['dri']
    for y in range(uy):
        for x in range(ux):
            if dri and unit and unit % dri == 0:
                br.restart(unit // dri - 1)             # numbered from 0 in every scan
                pred, eobrun = [0] * len(sc), 0
            unit += 1
            for k, (ci, td, ta) in enumerate(sc):
                c = comps[ci]
                nh, nv = (c['h'], c['v']) if inter else (1, 1)
                for v in range(nv):
                    for h in range(nh):
                        blk = c['coef'][y * nv + v, x * nh + h].tolist()
                        pred[k], eobrun = _block(br, kind, blk, st['ht'].get((0, td)), st['ht'].get((1, ta)), pred[k], ss, se, al, eobrun)
                        c['coef'][y * nv + v, x * nh + h] = blk
    return br.p


def coefficients(b, accept=ALL, header_only=False):
    """The whole file -> the dict jpeg_ref.coefficients() returns (comps[i]['coef'] int16 [block rows, block columns, 64],
    natural order, whole-MCU block counts; q[comps[i]['tq']] the table latched at the component's first scan), plus
    'progressive' and 'scans'.  header_only: stop at the first SOS, frame and first scan header checked."""
    b = bytes(b)
    if b[:2] != b'\xff\xd8' or len(b) < 4:
        raise JpegCorrupt('no SOI')
    st = dict(q={}, ht={}, dri=0, orient=None, jfif=False, adobe=None, comps=None, progressive=False)
    i, scans = 2, 0
    while True:
        if i + 2 > len(b) or b[i] != 0xFF:
            raise JpegCorrupt('marker expected')
        m = b[i + 1]
        i += 2
        if m == 0xFF:
            i -= 1
            continue
        if m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m == 0xD9 and scans:
            break
        if m in (0xD9, 0xD8, 0):
            raise JpegCorrupt('unexpected marker %02x' % m)
        if i + 2 > len(b):
            raise JpegCorrupt('truncated')
        L = struct.unpack('>H', b[i:i + 2])[0]
        if L < 2 or i + L > len(b):
            raise JpegCorrupt('truncated segment')
        s = b[i + 2:i + L]
        i += L
        if m in (0xC0, 0xC1, 0xC2):
            if m == 0xC2 and not accept & PROGRESSIVE:
                raise JpegUnsupported('progressive')
            if st['comps'] is not None or len(s) < 6:
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
            st.update(H=H, W=W, progressive=m == 0xC2,
                      comps=[dict(id=s[6 + 3 * k], h=s[7 + 3 * k] >> 4, v=s[7 + 3 * k] & 15, tq=s[8 + 3 * k]) for k in range(n)])
        elif m != 0xDA:
            _tables(m, s, st)
        else:
            if st['comps'] is None:
                raise JpegCorrupt('SOS before SOF')
            if scans == 0:
                _frame_checks(st, accept)
            scan = _scan_header(s, st, accept)
            if header_only:
                break
            scans += 1
            if scans > MAX_SCANS:
                raise JpegUnsupported('more than %d scans' % MAX_SCANS)
            for ci, _, _ in scan[0]:
                c = st['comps'][ci]
                if c['q'] is None:
                    c['q'] = st['q'][c['tq']].copy()
                for j in range(scan[1], scan[2] + 1):
                    c['bits'][j] = scan[4]
            i = _run_scan(b, i, st, scan)
    if not header_only:
        for c in st['comps']:
            if any(v != 0 for v in c['bits']):
                if st['progressive']:
                    raise JpegUnsupported('incomplete progressive scan script')
                raise JpegCorrupt('a component has no scan')
    q = {}
    for ci, c in enumerate(st['comps']):
        c['tq_file'], c['tq'] = c['tq'], ci                 # one latched table per component
        q[ci] = c.pop('q')
        c['coef'] = c['coef'].astype(np.int16)
        del c['bits']
    return dict(W=st['W'], H=st['H'], comps=st['comps'], q=q, dri=st['dri'], orientation=st['orient'] or 1, hmax=st['hmax'],
                vmax=st['vmax'], progressive=st['progressive'], scans=scans)


# ------------------------------------------------------------------------------------------------------------ upsamplers
def h1v2(p, n, m):
    """jdsample.c h1v2_fancy_upsample: a plane at half height and full width; rows 3/4 nearer + 1/4 further, the biases 1
    (upper output row) and 2 (lower), edges replicated at the downsampled height m."""
    p = p[:m, :n].astype(np.int64)
    up = np.concatenate([p[:1], p[:-1]])
    dn = np.concatenate([p[1:], p[-1:]])
    o = np.zeros((2 * m, n), np.int64)
    o[0::2] = (3 * p + up + 1) >> 2
    o[1::2] = (3 * p + dn + 2) >> 2
    return o


def upsample(p, fx, fy, dw, dh):
    """jdsample.c jinit_upsampler with fancy upsampling on: which upsampler serves the ratio fx x fy of a plane dw x dh."""
    if (fx, fy) == (1, 1):
        return p
    if (fx, fy) == (2, 1) and dw > 2:
        return R.h2v1(p, dw)
    if (fx, fy) == (2, 2) and dw > 2:
        return R.h2v2(p, dw, dh)
    if (fx, fy) == (1, 2):
        return h1v2(p, dw, dh)
    return np.repeat(np.repeat(p, fx, 1), fy, 0)            # h2v1 / h2v2 on a narrow plane, and int_upsample


def reconstruct(hd, apply_orientation=True):
    H, W = hd['H'], hd['W']
    hm, vm = max(c['h'] for c in hd['comps']), max(c['v'] for c in hd['comps'])
    pl = []
    for c in hd['comps']:
        dw, dh = -(-W * c['h'] // hm), -(-H * c['v'] // vm)
        pl.append(upsample(R.plane(c, hd['q']), hm // c['h'], vm // c['v'], dw, dh)[:H, :W].astype(np.int64))
    if len(pl) == 1:
        out = np.stack([pl[0]] * 3, -1).astype(np.uint8)
    else:                                                   # jdcolor.c, as in jpeg_ref.reconstruct
        y, cb, cr = pl
        x = np.arange(256) - 128
        r = np.clip(y + ((91881 * x + 32768) >> 16)[cr], 0, 255)
        g = np.clip(y + (((-22554 * x + 32768)[cb] + (-46802 * x)[cr]) >> 16), 0, 255)
        bl = np.clip(y + ((116130 * x + 32768) >> 16)[cb], 0, 255)
        out = np.stack([bl, g, r], -1).astype(np.uint8)
    return R.orient(out, hd['orientation']) if apply_orientation else out


def decode(b, accept=ALL, apply_orientation=True):
    return reconstruct(coefficients(b, accept), apply_orientation)
