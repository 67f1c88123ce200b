"""PNG files -> uint8 HWC BGR device tensors, the pixels cv2.imread(path) gives (reference demo.py:41, tools/cocotools.py:105,
tools/transform.py:87), pinned bit for bit to Pillow's libpng decode, `np.asarray(Image.open(f).convert('RGB'))[..., ::-1]`
(DESIGN.md section 10e names the one case where Pillow departs from the rule below and the numpy restatement alone is the pin).

Every colour type and bit depth of the PNG specification, Adam7 included: grey is replicated to B = G = R (depth 1 / 2 / 4
scaled by 255 / 85 / 17), a palette index is looked up in PLTE, an alpha channel is dropped (not composited), tRNS is
ignored, a 16-bit sample gives its high byte, and gAMA / sRGB / iCCP / cHRM / bKGD / pHYs / text / time chunks change nothing.

Host, in Python and testable without the library: signature, the chunk walk with zlib.crc32 over every chunk, IHDR and PLTE
validation, the concatenated IDAT data through zlib on a thread pool (zlib releases the interpreter lock; bounded output: a
small file cannot expand past the image it declares), and the filter-type byte of every scanline.  Device: everything per
byte, csrc/png.hip -- the five scanline filters reversed with the rows skewed over the lanes, expansion and the Adam7
scatter fused into the store.  One pinned staging buffer per call holds [descriptor table with the palettes | scanline
streams] and crosses in one copy; the launches follow without a host synchronisation.

A file outside the subset raises PPYoloHipError('item i: unsupported PNG: <reason>'), a damaged one 'item i: corrupt PNG:
<reason>'."""
import collections
import ctypes
import struct
import zlib

import numpy as np
import torch

from . import _lib
from ._lib import PPYoloHipError, lib
from ._lib import check as _check
from .hostio import MAX_THREADS      # noqa: F401 (re-exported)
from .hostio import HostPool, ImreadMixin, StagingRing, check_outputs, read_bytes, row_pitch

SIGNATURE = b'\x89PNG\r\n\x1a\n'
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
DEPTHS = {0: (1, 2, 4, 8, 16), 2: (8, 16), 3: (1, 2, 4, 8), 4: (8, 16), 6: (8, 16)}
ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))      # xs, ys, xd, yd


class Refusal(Exception):
    """kind 'unsupported' (a valid file for another decoder) or 'corrupt', and the reason."""

    def __init__(self, kind, reason):
        Exception.__init__(self, '%s PNG: %s' % (kind, reason))
        self.kind, self.reason = kind, reason


Header = collections.namedtuple('Header', 'width height depth ctype interlace palette idat passes expected')


def row_bytes(cols, ctype, depth):
    return (cols * CHANNELS[ctype] * depth + 7) // 8


def passes(width, height, ctype, depth, interlace):
    """The sub-images of the scanline stream in order, empty ones left out: [(xs, ys, xd, yd, cols, rows, row bytes)]."""
    if not interlace:
        return [(0, 0, 1, 1, width, height, row_bytes(width, ctype, depth))]
    out = []
    for xs, ys, xd, yd in ADAM7:
        cols, rows = (width - xs + xd - 1) // xd if width > xs else 0, (height - ys + yd - 1) // yd if height > ys else 0
        if cols and rows:
            out.append((xs, ys, xd, yd, cols, rows, row_bytes(cols, ctype, depth)))
    return out


def expected_bytes(width, height, ctype, depth, interlace):
    """Length of the inflated stream: over the non-empty passes, rows * (1 + ceil(cols * channels * depth / 8))."""
    return sum(p[5] * (1 + p[6]) for p in passes(width, height, ctype, depth, interlace))


def parse(data, max_pixels=1 << 28):
    """The chunk walk: signature, CRC of every chunk, IHDR, PLTE, the IDAT ranges, up to IEND (later bytes are ignored).
    Nothing is inflated and no buffer is sized.  -> Header; raises Refusal."""
    view = memoryview(data)
    if bytes(view[:8]) != SIGNATURE:
        raise Refusal('corrupt', 'bad signature')
    pos, end = 8, len(view)
    ihdr = palette = None
    idat, idat_closed = [], False
    while True:
        if pos == end:
            raise Refusal('corrupt', 'truncated: no IEND chunk')
        if end - pos < 8:
            raise Refusal('corrupt', 'truncated inside a chunk header')
        length, = struct.unpack_from('>I', view, pos)
        ctype = bytes(view[pos + 4:pos + 8])
        name = ctype.decode('latin-1')
        if not all(65 <= c <= 90 or 97 <= c <= 122 for c in ctype):
            raise Refusal('corrupt', 'chunk type %r is not four letters' % ctype)
        if length > 0x7fffffff or end - pos - 12 < length:
            raise Refusal('corrupt', 'truncated: chunk %s of %d bytes runs past the end of the file' % (name, length))
        body = view[pos + 8:pos + 8 + length]
        crc, = struct.unpack_from('>I', view, pos + 8 + length)
        if zlib.crc32(view[pos + 4:pos + 8 + length]) != crc:
            raise Refusal('corrupt', 'bad CRC in chunk %s' % name)
        if ihdr is None and ctype != b'IHDR':
            raise Refusal('corrupt', 'the first chunk is %s, not IHDR' % name)
        pos += 12 + length
        if ctype == b'IHDR':
            if ihdr is not None:
                raise Refusal('corrupt', 'a second IHDR chunk')
            if length != 13:
                raise Refusal('corrupt', 'IHDR of %d bytes' % length)
            ihdr = _check_ihdr(struct.unpack('>IIBBBBB', body), max_pixels)
        elif ctype == b'PLTE':
            if palette is not None:
                raise Refusal('corrupt', 'a second PLTE chunk')
            if idat:
                raise Refusal('corrupt', 'PLTE after IDAT')
            if length == 0 or length % 3 or length > 768:
                raise Refusal('corrupt', 'PLTE of %d bytes' % length)
            palette = bytes(body)
        elif ctype == b'IDAT':
            if idat_closed:
                raise Refusal('corrupt', 'IDAT chunks are not consecutive')
            if ihdr[3] == 3 and palette is None:
                raise Refusal('corrupt', 'missing PLTE')
            idat.append(body)
        elif ctype == b'IEND':
            break
        else:
            if not ctype[0] & 0x20:
                raise Refusal('unsupported', 'unknown critical chunk %s' % name)
            # ancillary: tRNS, gAMA, sRGB, iCCP, cHRM, bKGD, pHYs, tEXt / zTXt / iTXt, tIME, APNG's acTL / fcTL / fdAT, ...
        if idat and ctype != b'IDAT':
            idat_closed = True
    if not idat:
        raise Refusal('corrupt', 'no IDAT chunk')
    w, h, depth, ct, interlace = ihdr
    pal = palette if ct == 3 else b''
    return Header(w, h, depth, ct, interlace, pal, idat, passes(w, h, ct, depth, interlace), expected_bytes(w, h, ct, depth, interlace))


def _check_ihdr(f, max_pixels):
    w, h, depth, ct, comp, filt, interlace = f
    if w == 0 or h == 0 or w > 0x7fffffff or h > 0x7fffffff:
        raise Refusal('corrupt', 'width %d, height %d' % (w, h))
    if w > 65535 or h > 65535:
        raise Refusal('unsupported', '%d x %d pixels: a side is over 65535' % (w, h))
    if w * h > max_pixels:
        raise Refusal('unsupported', '%d x %d pixels is over max_pixels = %d' % (w, h, max_pixels))
    if ct not in DEPTHS:
        raise Refusal('corrupt', 'colour type %d' % ct)
    if depth not in (1, 2, 4, 8, 16):
        raise Refusal('corrupt', 'bit depth %d' % depth)
    if depth not in DEPTHS[ct]:
        raise Refusal('corrupt', 'bit depth %d with colour type %d' % (depth, ct))
    if comp != 0:
        raise Refusal('unsupported', 'compression method %d' % comp)
    if filt != 0:
        raise Refusal('unsupported', 'filter method %d' % filt)
    if interlace not in (0, 1):
        raise Refusal('unsupported', 'interlace method %d' % interlace)
    return w, h, depth, ct, interlace


def inflate(hdr):
    """The concatenated IDAT data through zlib, bounded to one byte more than the image needs -> bytes of exactly
    hdr.expected; raises Refusal('corrupt')."""
    src = hdr.idat[0] if len(hdr.idat) == 1 else b''.join(hdr.idat)
    try:
        raw = zlib.decompressobj().decompress(src, hdr.expected + 1)
    except zlib.error as e:
        raise Refusal('corrupt', 'zlib: %s' % e)
    if len(raw) > hdr.expected:
        raise Refusal('corrupt', 'the inflated data is longer than the %d bytes of the image' % hdr.expected)
    if len(raw) < hdr.expected:
        raise Refusal('corrupt', 'the inflated data ends after %d of %d bytes' % (len(raw), hdr.expected))
    return raw


def check_filters(raw, hdr):
    """The filter-type byte of every scanline, through a strided view; above 4 is Refusal('corrupt')."""
    flat = np.frombuffer(raw, np.uint8)
    off = 0
    for p in hdr.passes:
        rows, pitch = p[5], 1 + p[6]
        ft = flat[off:off + rows * pitch:pitch]
        if ft.max() > 4:
            r = int(np.argmax(ft > 4))
            raise Refusal('corrupt', 'filter type %d in row %d' % (ft[r], r))
        off += rows * pitch


class HostBatch(object):
    """Output of the host stage: descriptors + the pinned buffer holding [descriptor table | scanline streams].  It OWNS one of
    the decoder's two staging buffers until reconstruct() or release(), as jpeg.HostBatch does."""
    __slots__ = ('n', 'descs', 'sizes', 'stage', 'slot', 'gen', 'table_bytes', 'total_bytes')


class PngDecoder(ImreadMixin):
    def __init__(self, device='cuda', threads=None, max_pixels=1 << 28):
        """threads: workers of the host stage, default min(16, images of the call); never more than 16, never derived from
        the machine's CPU count.  max_pixels: a header that claims more is refused before any buffer is sized from it (a
        60-byte file can claim 65535 x 65535)."""
        self.device = torch.device(device)
        self._host = HostPool(threads, 'ppy-png')
        self.threads = self._host.threads
        self.max_pixels = int(max_pixels)
        self._ring = StagingRing(self.device, 1 << 20, stage='host')        # host_decode and reconstruct may run on two threads

    # ---- host stage ---------------------------------------------------------------------------------------------------
    def _staging(self, nbytes):
        return self._ring.take(nbytes)

    def release(self, hb):
        """Give back the staging buffer of a HostBatch that will not be reconstructed."""
        self._ring.release(hb.slot, hb.gen)

    def refusal(self, item):
        """The chunk walk only, nothing is inflated: None if decode() would take the item as far as its chunks tell, otherwise
        (kind, reason) with kind 'unsupported' or 'corrupt'.  Damage inside the IDAT data still surfaces in decode()."""
        try:
            parse(read_bytes(item), self.max_pixels)
        except Refusal as r:
            return r.kind, r.reason
        return None

    def host_decode(self, items):
        """Host only: walk, validate and inflate every item into a pinned staging buffer -> HostBatch (jpeg.JpegDecoder's
        entropy_decode: the batch owns the buffer until reconstruct(hb) or release(hb); may run on another thread)."""
        datas = [read_bytes(it) for it in items]
        n = len(datas)
        if n == 0:
            raise PPYoloHipError('empty batch')
        hdrs = []
        for i, d in enumerate(datas):
            try:
                hdrs.append(parse(d, self.max_pixels))
            except Refusal as r:
                raise PPYoloHipError('item %d: %s' % (i, r))
        table_bytes = (lib().ppy_png_table_bytes(n) + 15) // 16 * 16
        descs = (_lib.PngDesc * n)()
        total = table_bytes
        for d, h in zip(descs, hdrs):
            d.width, d.height, d.bit_depth, d.colour_type, d.interlace = h.width, h.height, h.depth, h.ctype, h.interlace
            d.palette_entries = len(h.palette) // 3
            ctypes.memmove(d.palette, h.palette, len(h.palette))
            d.scan_offset, d.scan_bytes = total - table_bytes, h.expected
            total += (h.expected + 15) // 16 * 16
        slot, gen, stage = self._staging(total)
        hb = HostBatch()
        hb.n, hb.descs, hb.stage, hb.slot, hb.gen, hb.table_bytes, hb.total_bytes = n, descs, stage, slot, gen, table_bytes, total
        hb.sizes = [(h.height, h.width) for h in hdrs]
        flat = stage.numpy()

        def one(i):
            try:
                raw = inflate(hdrs[i])
                check_filters(raw, hdrs[i])
            except Refusal as r:
                return r
            off = table_bytes + descs[i].scan_offset
            flat[off:off + len(raw)] = np.frombuffer(raw, np.uint8)
            return None

        try:
            for i, r in enumerate(self._host.map(one, n)):
                if r is not None:
                    raise PPYoloHipError('item %d: %s' % (i, r))
        except BaseException:
            self.release(hb)
            raise
        return hb

    # ---- device stage -------------------------------------------------------------------------------------------------
    def reconstruct(self, hb, out=None):
        """Copy a HostBatch to the device and enqueue the reconstruction on the current stream; nothing is read back.  out:
        optional list of uint8 device tensors [h,w,3] to fill (pixel stride 3, channel stride 1, any row pitch)."""
        L = lib()
        n = hb.n
        if out is None:
            out = [torch.empty((h, w, 3), dtype=torch.uint8, device=self.device) for h, w in hb.sizes]
        else:
            check_outputs(out, hb.sizes, self.device)
        with self._ring.uploading(hb.slot, hb.gen) as staging:
            _check(L.ppy_png_pack_table(n, hb.descs, (ctypes.c_void_p * n)(*[t.data_ptr() for t in out]),
                                        (ctypes.c_longlong * n)(*[row_pitch(t) for t in out]),
                                        hb.stage.data_ptr(), hb.table_bytes), 'ppy_png_pack_table')
            blob = staging.copy(hb.total_bytes)
        ws_bytes = L.ppy_png_workspace_bytes(n, hb.descs)
        ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=self.device)
        _check(L.ppy_png_reconstruct_u8(n, hb.descs, blob.data_ptr(), blob.data_ptr() + hb.table_bytes, hb.total_bytes - hb.table_bytes,
                                        ws.data_ptr(), ws_bytes, torch.cuda.current_stream().cuda_stream), 'ppy_png_reconstruct_u8')
        return out

    # ---- the user's calls ---------------------------------------------------------------------------------------------
    def decode(self, items, out=None):
        """list of bytes / memoryview / paths -> list of uint8 [h,w,3] BGR device tensors, asynchronous on the current stream."""
        hb = self.host_decode(items)
        try:
            return self.reconstruct(hb, out=out)
        except BaseException:
            self.release(hb)                # (outputs refused: the batch never reached the device)
            raise
