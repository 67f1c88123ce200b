"""A PNG WRITER for tests, on struct + zlib alone: any colour type and bit depth, a chosen filter type per row, Adam7, PLTE /
tRNS, extra chunks, IDAT split sizes and deliberate damage.  It writes what it is told to, valid or not."""
import struct
import zlib

import numpy as np

SIGNATURE = b'\x89PNG\r\n\x1a\n'
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))      # xs, ys, xd, yd


def chunk(ctype, body=b'', crc=None):
    """One chunk; crc: the value to store instead of the right one."""
    c = zlib.crc32(ctype + body) if crc is None else crc
    return struct.pack('>I', len(body)) + ctype + body + struct.pack('>I', c & 0xffffffff)


def ihdr(width, height, depth, ctype, interlace=0, compression=0, filter_method=0):
    return chunk(b'IHDR', struct.pack('>IIBBBBB', width, height, depth, ctype, compression, filter_method, interlace))


def pack_rows(samples, depth):
    """samples [rows, cols, channels] of ints below 2 ** depth -> uint8 [rows, row bytes] as PNG stores them."""
    rows, cols, ch = samples.shape
    s = samples.reshape(rows, cols * ch).astype(np.uint32)
    if depth == 16:
        out = np.empty((rows, cols * ch, 2), np.uint8)
        out[..., 0], out[..., 1] = s >> 8, s & 255
        return out.reshape(rows, -1)
    if depth == 8:
        return s.astype(np.uint8)
    per = 8 // depth
    pad = (-s.shape[1]) % per
    s = np.concatenate([s, np.zeros((rows, pad), np.uint32)], 1).reshape(rows, -1, per)
    out = np.zeros(s.shape[:2], np.uint32)
    for q in range(per):
        out |= s[..., q] << (8 - depth * (q + 1))
    return out.astype(np.uint8)


def filter_row(ft, cur, prev, bpp):
    """Filter type ft applied to the raw row `cur` (uint8) with the raw row above `prev` (zeros for the first row)."""
    cur, prev = cur.astype(np.int32), prev.astype(np.int32)
    a = np.concatenate([np.zeros(bpp, np.int32), cur[:-bpp]]) if len(cur) > bpp else np.zeros_like(cur)
    c = np.concatenate([np.zeros(bpp, np.int32), prev[:-bpp]]) if len(cur) > bpp else np.zeros_like(cur)
    a, c = a[:len(cur)], c[:len(cur)]
    if ft == 0:
        pred = 0
    elif ft == 1:
        pred = a
    elif ft == 2:
        pred = prev
    elif ft == 3:
        pred = (a + prev) >> 1
    else:
        p = a + prev - c
        pa, pb, pc = abs(p - a), abs(p - prev), abs(p - c)
        pred = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, prev, c))
    return ((cur - pred) & 255).astype(np.uint8)


def scanlines(samples, ctype, depth, filters=0, interlace=0):
    """The scanline stream (before zlib).  filters: one type, a list cycled over the rows of each pass, or f(pass, row)."""
    h, w, _ = samples.shape
    bpp = max(1, CHANNELS[ctype] * depth // 8)
    out = []
    for p, (xs, ys, xd, yd) in enumerate(ADAM7 if interlace else ((0, 0, 1, 1),)):
        sub = samples[ys::yd, xs::xd]
        if sub.shape[0] == 0 or sub.shape[1] == 0:
            continue
        rows = pack_rows(sub, depth)
        prev = np.zeros(rows.shape[1], np.uint8)
        for r in range(rows.shape[0]):
            ft = filters(p, r) if callable(filters) else filters[r % len(filters)] if isinstance(filters, (list, tuple)) else filters
            out.append(bytes([ft]) + (filter_row(ft, rows[r], prev, bpp).tobytes() if ft <= 4 else rows[r].tobytes()))
            prev = rows[r]
    return b''.join(out)


def split_idat(z, sizes):
    """z cut into IDAT chunks of the given sizes in turn (0 = an empty chunk); what is left goes into a last one."""
    out, pos = [], 0
    for n in sizes or ():
        out.append(chunk(b'IDAT', z[pos:pos + n]))
        pos += n
    if pos < len(z) or not out:
        out.append(chunk(b'IDAT', z[pos:]))
    return out


def make_png(samples, ctype, depth, filters=0, interlace=0, palette=None, before_idat=(), after_idat=(), idat_sizes=None, level=6,
             stream=None, tail=b''):
    """samples: int array [h, w, channels].  palette: bytes for PLTE.  before_idat / after_idat: ready-made chunks (tRNS, gAMA,
    ...).  stream: the scanline stream to compress instead of the one the samples give (damage)."""
    samples = np.asarray(samples)
    h, w, _ = samples.shape
    raw = scanlines(samples, ctype, depth, filters, interlace) if stream is None else stream
    parts = [SIGNATURE, ihdr(w, h, depth, ctype, interlace)]
    if palette is not None:
        parts.append(chunk(b'PLTE', bytes(palette)))
    parts += list(before_idat) + split_idat(zlib.compress(raw, level), idat_sizes) + list(after_idat) + [chunk(b'IEND'), tail]
    return b''.join(parts)


def random_samples(rng, h, w, ctype, depth, two_valued=False, palette_entries=None):
    top = (palette_entries if ctype == 3 and palette_entries else 1 << depth)
    if two_valued:
        return rng.choice([0, top - 1], size=(h, w, CHANNELS[ctype]))
    return rng.randint(0, top, (h, w, CHANNELS[ctype]))
