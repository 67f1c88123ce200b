"""The numpy restatement of the PNG pixel contract: inflate, unfilter, de-interlace, expand to BGR.
Written for clarity, byte by byte; it shares no code with ppyolo_hip/png.py or csrc/png.hip.

The rules: grey replicated to B = G = R (depth 1 / 2 / 4 scaled by 255 / 85 / 17); a palette index looked up in PLTE (an index
at or past its end: black); alpha dropped; tRNS and every other ancillary chunk ignored; a 16-bit sample gives its high byte."""
import struct
import zlib

import numpy as np

CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))      # xs, ys, xd, yd


def chunks(data):
    pos = 8
    while pos + 12 <= len(data):
        n, = struct.unpack_from('>I', data, pos)
        yield data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        if data[pos + 4:pos + 8] == b'IEND':
            return
        pos += 12 + n


def paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    if pa <= pb and pa <= pc:
        return a
    return b if pb <= pc else c


def unfilter(raw, rows, rb, bpp):
    """rows scanlines of 1 + rb bytes -> uint8 [rows, rb] reconstructed."""
    out = np.zeros((rows, rb), np.uint8)
    prev = [0] * rb
    for r in range(rows):
        line = raw[r * (rb + 1):(r + 1) * (rb + 1)]
        ft, cur = line[0], [0] * rb
        for i in range(rb):
            a = cur[i - bpp] if i >= bpp else 0
            b = prev[i]
            c = prev[i - bpp] if i >= bpp else 0
            pred = (0, a, b, (a + b) >> 1, paeth(a, b, c))[ft]
            cur[i] = (line[1 + i] + pred) & 255
        out[r] = cur
        prev = cur
    return out


def expand(rows, cols, ctype, depth, palette):
    """uint8 [rows, row bytes] reconstructed -> uint8 [rows, cols, 3] BGR."""
    n = rows.shape[0]
    ch = CHANNELS[ctype]
    if depth < 8:
        per = 8 // depth
        bits = np.stack([(rows >> (8 - depth * (q + 1))) & ((1 << depth) - 1) for q in range(per)], -1).reshape(n, -1)[:, :cols]
        s = bits.reshape(n, cols, 1)
        if ctype == 0:
            s = s * (255 // ((1 << depth) - 1))
    elif depth == 8:
        s = rows.reshape(n, cols, ch)
    else:
        s = rows.reshape(n, cols, ch, 2)[..., 0]      # the high byte
    s = s.astype(np.uint8)
    if ctype == 3:
        pal = np.zeros((256, 3), np.uint8)
        pal[:len(palette) // 3] = np.frombuffer(palette, np.uint8).reshape(-1, 3)
        rgb = pal[s[..., 0]]
    elif ctype in (0, 4):
        rgb = np.repeat(s[..., :1], 3, -1)
    else:
        rgb = s[..., :3]
    return np.ascontiguousarray(rgb[..., ::-1])


def decode(data):
    """A PNG file -> uint8 [h, w, 3] BGR."""
    data = bytes(data)
    palette, idat = b'', []
    for t, body in chunks(data):
        if t == b'IHDR':
            w, h, depth, ctype, _, _, interlace = struct.unpack('>IIBBBBB', body)
        elif t == b'PLTE':
            palette = body
        elif t == b'IDAT':
            idat.append(body)
    raw = zlib.decompress(b''.join(idat))
    bpp = max(1, CHANNELS[ctype] * depth // 8)
    out = np.zeros((h, w, 3), np.uint8)
    pos = 0
    for xs, ys, xd, yd in (ADAM7 if interlace else ((0, 0, 1, 1),)):
        cols, rows = len(range(xs, w, xd)), len(range(ys, h, yd))
        if cols == 0 or rows == 0:
            continue
        rb = (cols * CHANNELS[ctype] * depth + 7) // 8
        out[ys::yd, xs::xd] = expand(unfilter(raw[pos:pos + rows * (rb + 1)], rows, rb, bpp), cols, ctype, depth, palette)
        pos += rows * (rb + 1)
    return out
