"""Write pytorch-ppyolo_amd/ppyolo_hip/label_font.py from Pillow's built-in bitmap font.

    python tools/make_label_font.py [--check]

Pillow's `ImageFont.load_default_imagefont()` is a PILfont: 256 glyph records of ten big-endian int16 (dx, dy, destination
x0 y0 x1 y1 relative to the pen on the baseline, source x0 y0 x1 y1 in the atlas) and a 1-bit atlas image.  `getmask(text)`
makes a band `sum(dx)` wide and `max(y1) - min(y0)` high, puts the baseline at row `-min(y0)` and PASTES each glyph's source
rectangle onto its destination rectangle in string order, overwriting what is there (set and clear bits alike).  This tool
keeps, for the printable ASCII characters 32..126, the destination rectangle relative to the glyph's own 6 x 11 cell and the
bits of its source rectangle; the package reads them as plain data and never imports Pillow.
--check compares the committed file with what the installed Pillow gives and exits 1 if they differ."""
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'pytorch-ppyolo_amd', 'ppyolo_hip', 'label_font.py')
FIRST, LAST = 32, 126
CELL_W, CELL_H, BASELINE = 6, 11, 9


def pilfont():
    """(metrics, atlas): 256 tuples of ten ints and the atlas as a list of rows of 0/1, from the installed Pillow."""
    from PIL import ImageFont
    got = []
    orig = ImageFont.ImageFont._load

    def capture(self, image, data):
        got.append((image, data))
        return orig(self, image, data)

    ImageFont.ImageFont._load = capture
    try:
        ImageFont.load_default_imagefont()
    finally:
        ImageFont.ImageFont._load = orig
    image, data = got[0]
    assert len(data) == 256 * 20, len(data)
    metrics = [struct.unpack('>10h', data[20 * i:20 * i + 20]) for i in range(256)]
    image = image.convert('L')
    w, h = image.size
    px = image.tobytes()
    atlas = [[1 if px[y * w + x] else 0 for x in range(w)] for y in range(h)]
    return metrics, atlas


def extract():
    """(rects, bitmaps) of characters 32..126: rects[i] = (gx0, gy0, gx1, gy1), the destination rectangle inside the glyph's
    cell (columns relative to the cell's left edge, rows from the top of the 11-row band); bitmaps[i] = one int per row of the
    rectangle, bit k = column gx0 + k."""
    metrics, atlas = pilfont()
    used = [m for m in metrics if m[4] > m[2] and m[5] > m[3]]
    assert -min(m[3] for m in used) == BASELINE and max(m[5] for m in used) + BASELINE == CELL_H
    rects, bitmaps = [], []
    for ch in range(FIRST, LAST + 1):
        dx, dy, x0, y0, x1, y1, sx0, sy0, sx1, sy1 = metrics[ch]
        assert (dx, dy) == (CELL_W, 0), (ch, dx, dy)
        assert sx1 - sx0 == x1 - x0 and sy1 - sy0 == y1 - y0, ch           # Pillow pastes without scaling
        assert -1 <= x0 <= x1 <= CELL_W and 0 <= y0 + BASELINE <= y1 + BASELINE <= CELL_H, (ch, x0, y0, x1, y1)
        rects.append((x0, y0 + BASELINE, x1, y1 + BASELINE))
        bitmaps.append(tuple(sum(atlas[sy][sx0 + k] << k for k in range(x1 - x0)) for sy in range(sy0, sy1)))
    return rects, bitmaps


def render(rects, bitmaps):
    lines = ['"""The label font of ppyolo_hip.draw: Pillow\'s built-in bitmap font (ImageFont.load_default_imagefont, courB08) as plain',
             'data, written by tools/make_label_font.py -- do not edit.  A monospace font of 6 x 11 cells; glyph i of a string owns the',
             'destination rectangle [6 i + gx0, 6 i + gx1) x [gy0, gy1) of the 11-row band and a bitmap of that size, the glyphs are',
             'pasted in string order and a pixel takes the bit of the LAST glyph whose rectangle contains it (gx0 is -1 for 29 glyphs:',
             'they reach back into column 5 of the cell before).  These are NOT OpenCV\'s Hershey glyphs.  DESIGN.md section 10c."""',
             'FIRST, LAST = %d, %d          # characters covered; any other is drawn as \'?\'' % (FIRST, LAST),
             'CELL_W, CELL_H = %d, %d' % (CELL_W, CELL_H),
             '# (gx0, gy0, gx1, gy1) per character',
             'RECTS = (']
    for i in range(0, len(rects), 6):
        lines.append('    ' + ' '.join('(%d, %d, %d, %d),' % r for r in rects[i:i + 6]))
    lines += [')', '# one int per row of the rectangle, bit k = column gx0 + k', 'BITMAPS = (']
    for i, b in enumerate(bitmaps):
        lines.append('    (%s),%s' % (' '.join('%d,' % v for v in b), '' if b else '          # %r' % chr(FIRST + i)))
    lines += [')', '', '',
              'def glyph(ch):',
              '    """(rect, bitmap) of a character code."""',
              '    i = ch - FIRST if FIRST <= ch <= LAST else ord(\'?\') - FIRST',
              '    return RECTS[i], BITMAPS[i]',
              '', '',
              'def text_mask(codes):',
              '    """The band of a string as rows of 0/1, CELL_H x CELL_W * len(codes): what Pillow\'s font.getmask gives."""',
              '    band = [[0] * (CELL_W * len(codes)) for _ in range(CELL_H)]',
              '    for i, ch in enumerate(codes):',
              '        (x0, y0, x1, y1), bits = glyph(ch)',
              '        for y in range(y0, y1):',
              '            for x in range(x0, x1):',
              '                if 0 <= CELL_W * i + x < len(band[0]):',
              '                    band[y][CELL_W * i + x] = bits[y - y0] >> (x - x0) & 1',
              '    return band',
              '', '',
              'def device_table():',
              '    """bytes, 16 per character: gx0 + 1, gy0, gx1 + 1, gy1, 0, then the 11 rows of the band, bit c + 1 = column c of the cell',
              '    (-1 <= c < 6) -- the layout csrc/draw.hip reads."""',
              '    out = bytearray()',
              '    for (x0, y0, x1, y1), bits in zip(RECTS, BITMAPS):',
              '        rows = [0] * CELL_H',
              '        for y in range(y0, y1):',
              '            rows[y] = bits[y - y0] << (x0 + 1)',
              '        out += bytes([x0 + 1, y0, x1 + 1, y1, 0] + rows)',
              '    return bytes(out)',
              '']
    return '\n'.join(lines)


if __name__ == '__main__':
    text = render(*extract())
    if '--check' in sys.argv:
        same = os.path.exists(OUT) and open(OUT).read() == text
        print('label_font.py is %s' % ('up to date' if same else 'STALE'))
        sys.exit(0 if same else 1)
    with open(OUT, 'w') as fh:
        fh.write(text)
    print('wrote %s (%d glyphs)' % (OUT, LAST - FIRST + 1))
