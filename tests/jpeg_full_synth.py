"""Writers from coefficients for the files JpegDecoder(accept=...) adds, on top of jpeg_synth: any accepted sampling, sequential
files in several scans, and progressive files from a scan script (the encoder side of libjpeg's jcphuff.c, without its
statistics pass: the Huffman tables are fixed).  Nothing here runs a forward DCT: synth() draws the coefficients (jpeg_synth's
`natural` regime: every block stays in zone A, so every libjpeg-turbo build decodes the same pixels) and the writers code
exactly those.

    synth(rng, H, W, luma, orientation)   luma = (h, v) of component 0 (chroma 1x1), or 'grey'
    sequential(hd, groups, ...)           one scan per group of component indices: [[0], [1], [2]], [[0], [1, 2]], [[2, 0, 1]]
    progressive(hd, script, ...)          script = [(component indices, Ss, Se, Ah, Al), ...]
A single-scan file of any sampling is jpeg_synth.encode(hd)."""
import struct

import numpy as np

import jpeg_ref as R
import jpeg_synth as S

# the luma factors PPY_JPEG_ACCEPT_SAMPLING adds, by their usual names where they have one
NEW_LUMA = {'440': (1, 2), '411': (4, 1), '410': (4, 2), '1x4': (1, 4), '3x1': (3, 1), '2x4': (2, 4), '3x2': (3, 2), '1x3': (1, 3)}


def synth(rng, H, W, luma, orientation=1):
    samp = [(1, 1)] if luma == 'grey' else [tuple(luma), (1, 1), (1, 1)]
    hm, vm = samp[0]
    mx, my = -(-W // (8 * hm)), -(-H // (8 * vm))
    comps, q = [], {}
    for ci, (h, v) in enumerate(samp):
        q[ci] = S.quant_table(rng, rng.random() < 1 / 3)
        bh, bw = my * v, mx * h
        coef = S._blocks(rng, bh * bw, q[ci], 'natural', True)
        comps.append(dict(id=ci + 1, h=h, v=v, tq=ci, td=min(ci, 1), ta=min(ci, 1), coef=coef.astype(np.int16).reshape(bh, bw, 64)))
    return dict(W=W, H=H, comps=comps, q=q, dri=0, orientation=orientation, hmax=hm, vmax=vm)


def clear_padding(hd):
    """Zero the blocks that hold no image sample: a scan of one component never carries them, so a decoder leaves them zero."""
    for c in hd['comps']:
        bw, bh = real_blocks(hd, c)
        c['coef'][bh:] = 0
        c['coef'][:, bw:] = 0
    return hd


def real_blocks(hd, c):
    return -(-(-(-hd['W'] * c['h'] // hd['hmax'])) // 8), -(-(-(-hd['H'] * c['v'] // hd['vmax'])) // 8)


# ---------------------------------------------------------------------------------------------------------------- tables
# AC tables of a progressive file also code the end-of-band runs EOB0..EOB14 (r << 4, r = 0..14): 176 symbols.
_AC_SYMS = [r << 4 for r in range(16)] + [r << 4 | s for r in range(16) for s in range(1, 11)]


def _rank(rs):
    return ((rs >> 4) if rs & 15 == 0 and rs != 0xF0 else (rs >> 4) + (rs & 15) + 1, rs)


TABLES = {
    'flat': {(0, 0): S.TABLES['flat'][(0, 0)], (0, 1): S.TABLES['flat'][(0, 1)],
             (1, 0): S._spec([0] * 7 + [176] + [0] * 8, _AC_SYMS), (1, 1): S._spec([0] * 7 + [100, 76] + [0] * 7, _AC_SYMS[::-1])},
    # symbols at every length up to 16: the decoder's path past its 9-bit lookahead runs in every kind of scan
    'skewed': {(0, 0): S.TABLES['skewed'][(0, 0)], (0, 1): S.TABLES['skewed'][(0, 1)],
               (1, 0): S._spec([0, 1, 1, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2, 156], sorted(_AC_SYMS, key=_rank)),
               (1, 1): S._spec([0, 0, 2, 2, 2, 2, 2, 2, 2, 3, 3, 3, 3, 3, 3, 144], sorted(_AC_SYMS, key=lambda rs: (_rank(rs)[0], -rs)))},
}


# --------------------------------------------------------------------------------------------------------------- scripts
def script_default(ncomp):
    """jcparam.c jpeg_simple_progression: 10 scans for YCbCr, 6 for grey."""
    if ncomp == 1:
        return [((0,), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1), ((0,), 0, 0, 1, 0), ((0,), 1, 63, 1, 0)]
    return [((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1), ((0,), 6, 63, 0, 2),
            ((0,), 1, 63, 2, 1), ((0, 1, 2), 0, 0, 1, 0), ((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0)]


def script_spectral(ncomp):
    """Spectral selection only, the DC of each component in a scan of its own."""
    out = [((c,), 0, 0, 0, 0) for c in range(ncomp)]
    for c in range(ncomp):
        out += [((c,), 1, 10, 0, 0), ((c,), 11, 63, 0, 0)]
    return out


def script_deep(ncomp):
    """Two successive-approximation refinements on both DC (interleaved) and AC."""
    every = tuple(range(ncomp))
    out = [(every, 0, 0, 0, 2)] + [((c,), 1, 63, 0, 2) for c in range(ncomp)] + [(every, 0, 0, 2, 1)]
    out += [((c,), 1, 63, 2, 1) for c in range(ncomp)] + [(every, 0, 0, 1, 0)] + [((c,), 1, 63, 1, 0) for c in range(ncomp)]
    return out


def script_incomplete(ncomp):
    return script_default(ncomp)[:-1]               # luma's AC never reaches Al = 0


SCRIPTS = {'default': script_default, 'spectral': script_spectral, 'deep': script_deep}


# ---------------------------------------------------------------------------------------------------------------- writer
class _Bits(object):
    def __init__(self, out, stats):
        self.out, self.acc, self.n, self.stats = out, 0, 0, stats

    def put(self, v, n):
        self.acc = self.acc << n | v
        self.n += n

    def sym(self, table, s):
        code, ln = table[s]
        self.put(code, ln)
        if self.stats is not None:
            self.stats['len%d' % ln] = self.stats.get('len%d' % ln, 0) + 1

    def value(self, v, s):
        self.put(v if v >= 0 else v + (1 << s) - 1, s)

    def flush(self):
        pad = -self.n % 8
        self.put((1 << pad) - 1, pad)
        self.out.append(self.acc.to_bytes(self.n // 8, 'big').replace(b'\xff', b'\xff\0'))
        self.acc = self.n = 0


def _header(hd, sof, tables, early):
    comps = hd['comps']
    out = [b'\xff\xd8', S._seg(0xE0, b'JFIF\0\1\1\0\0\1\0\1\0\0')]
    if hd['orientation'] != 1:
        tiff = b'MM\0*' + struct.pack('>IH', 8, 1) + struct.pack('>HHIHH', 0x0112, 3, 1, hd['orientation'], 0) + struct.pack('>I', 0)
        out.append(S._seg(0xE1, b'Exif\0\0' + tiff))
    for tq in sorted(set(c['tq'] for c in comps)):
        out.append(_dqt(tq, hd['q'][tq]))
    out.append(S._seg(sof, struct.pack('>BHHB', 8, hd['H'], hd['W'], len(comps)) +
                      b''.join(bytes([c['id'], c['h'] << 4 | c['v'], c['tq']]) for c in comps)))
    for key in early:
        out.append(_dht(tables, key))
    return out


def _dqt(tq, table):
    t = np.asarray(table)[R.ZZ]
    pq = int(t.max() > 255)
    return S._seg(0xDB, bytes([pq << 4 | tq]) + t.astype('>u2' if pq else 'u1').tobytes())


def _dht(tables, key):
    bits, syms = TABLES[tables][key]
    return S._seg(0xC4, bytes([key[0] << 4 | key[1]]) + bytes(bits) + bytes(syms))


def _units(hd, cis):
    """The blocks of a scan in coding order: [[(component slot, block row, block column), ...] per unit] -- MCUs of an
    interleaved scan, otherwise the blocks of the one component that hold image samples."""
    comps = hd['comps']
    if len(cis) > 1:
        mx, my = -(-hd['W'] // (8 * hd['hmax'])), -(-hd['H'] // (8 * hd['vmax']))
        return [[(k, y * comps[ci]['v'] + v, x * comps[ci]['h'] + h) for k, ci in enumerate(cis)
                 for v in range(comps[ci]['v']) for h in range(comps[ci]['h'])] for y in range(my) for x in range(mx)]
    bw, bh = real_blocks(hd, comps[cis[0]])
    return [[(0, y, x)] for y in range(bh) for x in range(bw)]


def _write(hd, sof, scans, dri, tables, stats, late_tables, requant=None):
    """scans: [(component indices, Ss, Se, Ah, Al)]; sof 0xC0 = every scan sequential.  dri: one restart interval for the file
    or one per scan (a DRI segment goes before each scan whose interval changes).  late_tables: the AC tables are defined
    between the scans, just before the first scan that needs them.  requant: {scan index: (tq, table)}: a DQT segment before
    that scan, which must not change a component whose first scan has started."""
    comps = hd['comps']
    prog = sof == 0xC2
    keys = sorted(set((0, c['td']) for c in comps) | set((1, c['ta']) for c in comps))
    early = [k for k in keys if not (late_tables and prog and k[0] == 1)]
    out = _header(hd, sof, tables, early)
    defined = set(early)
    codes = {k: S._codes(TABLES[tables][k]) for k in keys}
    zz = R.ZZ.tolist()
    blocks = [c['coef'].astype(np.int64)[:, :, zz].tolist() for c in comps]            # zigzag order
    dris = list(dri) if isinstance(dri, (list, tuple)) else [dri] * len(scans)
    cur_dri = 0
    for si, (cis, ss, se, ah, al) in enumerate(scans):
        if requant and si in requant:
            out.append(_dqt(*requant[si]))
        for ci in cis:
            k = (1, comps[ci]['ta'])
            if k not in defined and ss > 0:
                out.append(_dht(tables, k))
                defined.add(k)
        if dris[si] != cur_dri:
            out.append(S._seg(0xDD, struct.pack('>H', dris[si])))
            cur_dri = dris[si]
        out.append(S._seg(0xDA, bytes([len(cis)]) + b''.join(bytes([comps[ci]['id'], comps[ci]['td'] << 4 | comps[ci]['ta']]) for ci in cis) +
                          bytes([ss, se, ah << 4 | al])))
        w = _Bits(out, stats)
        pred = [0] * len(cis)
        st = dict(eobrun=0, be=[])               # the pending end-of-band run and the correction bits that follow it

        def emit_eobrun(ac):
            if st['eobrun'] > 0:
                nb = st['eobrun'].bit_length() - 1
                w.sym(ac, nb << 4)
                if nb:
                    w.put(st['eobrun'] & ((1 << nb) - 1), nb)
                if stats is not None:
                    stats['eobrun_max'] = max(stats.get('eobrun_max', 0), st['eobrun'])
                st['eobrun'] = 0
            for bit in st['be']:
                w.put(bit, 1)
            st['be'] = []

        for u, unit in enumerate(_units(hd, cis)):
            if cur_dri and u and u % cur_dri == 0:
                if prog and ss > 0:
                    emit_eobrun(codes[(1, comps[cis[0]]['ta'])])
                w.flush()
                out.append(bytes([0xFF, 0xD0 + (u // cur_dri - 1) % 8]))
                pred = [0] * len(cis)
            for k, by, bx in unit:
                c = comps[cis[k]]
                b = blocks[cis[k]][by][bx]
                dc, ac = codes.get((0, c['td'])), codes.get((1, c['ta']))
                if not prog or (ss == 0 and ah == 0):                       # DC, sequential or first
                    v = b[0] >> al
                    d = v - pred[k]
                    pred[k] = v
                    s = S._size(d)
                    assert s <= 11
                    w.sym(dc, s)
                    w.value(d, s)
                if not prog:                                                # the AC of a sequential block
                    run = 0
                    for j in range(1, 64):
                        a = b[j]
                        if a == 0:
                            run += 1
                            continue
                        while run > 15:
                            w.sym(ac, 0xF0)
                            run -= 16
                        w.sym(ac, run << 4 | S._size(a))
                        w.value(a, S._size(a))
                        run = 0
                    if run:
                        w.sym(ac, 0x00)
                elif ss == 0 and ah:                                        # DC refinement: the next bit
                    w.put(b[0] >> al & 1, 1)
                elif ss > 0 and ah == 0:                                    # jcphuff.c encode_mcu_AC_first
                    run = 0
                    for j in range(ss, se + 1):
                        a = abs(b[j]) >> al
                        if a == 0:
                            run += 1
                            continue
                        emit_eobrun(ac)
                        while run > 15:
                            w.sym(ac, 0xF0)
                            run -= 16
                        s = S._size(a)
                        w.sym(ac, run << 4 | s)
                        w.value(a if b[j] > 0 else -a, s)
                        run = 0
                    if run:
                        st['eobrun'] += 1
                        if st['eobrun'] == 0x7FFF:
                            emit_eobrun(ac)
                elif ss > 0:                                                # jcphuff.c encode_mcu_AC_refine
                    absv = [abs(b[j]) >> al for j in range(se + 1)]
                    eob = max([j for j in range(ss, se + 1) if absv[j] == 1], default=0)
                    run, br = 0, []
                    for j in range(ss, se + 1):
                        t = absv[j]
                        if t == 0:
                            run += 1
                            continue
                        while run > 15 and j <= eob:
                            emit_eobrun(ac)
                            w.sym(ac, 0xF0)
                            run -= 16
                            for bit in br:
                                w.put(bit, 1)
                            br = []
                        if t > 1:
                            br.append(t & 1)
                            continue
                        emit_eobrun(ac)
                        w.sym(ac, run << 4 | 1)
                        w.put(0 if b[j] < 0 else 1, 1)
                        for bit in br:
                            w.put(bit, 1)
                        br = []
                        run = 0
                    if run or br:
                        st['eobrun'] += 1
                        st['be'] += br
                        if st['eobrun'] == 0x7FFF or len(st['be']) > 937:
                            emit_eobrun(ac)
        if prog and ss > 0:
            emit_eobrun(codes[(1, comps[cis[0]]['ta'])])
        w.flush()
    out.append(b'\xff\xd9')
    return b''.join(out)


def sequential(hd, groups, dri=0, tables='flat', stats=None):
    return _write(hd, 0xC0, [(tuple(g), 0, 63, 0, 0) for g in groups], dri, tables, stats, False)


def progressive(hd, script, dri=0, tables='flat', stats=None, late_tables=True, requant=None):
    return _write(hd, 0xC2, script, dri, tables, stats, late_tables, requant)
