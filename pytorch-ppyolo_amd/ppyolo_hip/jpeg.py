"""JPEG files -> uint8 HWC BGR device tensors, the pixels cv2.imread / cv2.imdecode(buf, 1) give (reference demo.py:41,
tools/cocotools.py:105, tools/transform.py:87), bit for bit with libjpeg-turbo's defaults wherever a block's inverse DCT
stays in [-512, 511], as every encoder's output does; beyond it, libjpeg's C arithmetic.

Host: marker parsing + Huffman decoding into coefficient blocks, plain C++ in the library (csrc/jpeg.hip), one call per image
on a thread pool -- ctypes releases the GIL.  Device: everything per pixel, two launches per batch (ops are in the library,
there is no fallback).  The coefficients are written straight into one of two pinned staging buffers and cross to the device
in one copy together with the descriptor table, so the entropy stage of the next batch overlaps the copy and the kernels of
this one.

JpegDecoder(entropy='device') moves the Huffman decoding to the GPU as well: the host keeps one linear pass per file (markers,
unstuffing, cutting at the restart markers: ppy_jpeg_scan_prepare), the compressed bytes cross instead of the coefficients,
and csrc/jpeg_entropy.hip fills the same coefficient buffer on the device, element for element.  Damage inside the entropy
data is then found on the device and comes back as one status word per image.  The default stays 'host'.

By default baseline Huffman JPEG only (grey or YCbCr 4:4:4 / 4:2:2 / 4:2:0, one interleaved scan): anything else raises
PPYoloHipError naming the reason, so a caller can hand that file to a decoder of its own.  JpegDecoder(accept='all') also takes
progressive files, sequential files in several scans and the luma factors of 4:4:0 / 4:1:1 / 4:1:0 and their like (host entropy
stage; the same two launches); arithmetic coding, 12-bit, CMYK / RGB and chroma factors other than 1x1 stay refused.  A
truncated or damaged file is an error too (libjpeg would fill the missing part with grey and warn).

JpegEncoder is the same codec run the other way: uint8 device images -> the bytes libjpeg-turbo writes with its defaults
(cv2.imwrite, reference demo.py:50; Pillow's Image.save), byte for byte.  Both stages run on the device
(csrc/jpeg_encode.hip): pixels -> the coefficient buffer the decoder defines -> entropy-coded bytes; the host writes the
headers and reads lengths and bytes back (two copies, one stream wait per call)."""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import PPYoloHipError, lib
from ._lib import check as _check
from .hostio import MAX_THREADS      # noqa: F401 (re-exported)
from .hostio import HostPool, ImreadMixin, Staging, StagingRing, check_image, check_outputs, read_bytes, row_pitch


def _refuse(i, rc, reason):
    kind = {-2: 'unsupported JPEG', -5: 'corrupt JPEG'}.get(rc, lib().ppy_error_string(rc).decode())
    return PPYoloHipError('item %d: %s: %s (code %d)' % (i, kind, reason.decode(errors='replace') or '?', rc))


def _accept_mask(accept):
    """'baseline' | 'all' | a subset of {'progressive', 'multiscan', 'sampling'} -> the PPY_JPEG_ACCEPT_* mask."""
    if accept == 'baseline':
        return 0
    names = set(_lib.JPEG_ACCEPT) if accept == 'all' else {accept} if isinstance(accept, str) else set(accept)
    if not names <= set(_lib.JPEG_ACCEPT):
        raise PPYoloHipError("accept must be 'baseline', 'all' or a subset of %s, got %r" % (sorted(_lib.JPEG_ACCEPT), accept))
    return sum(_lib.JPEG_ACCEPT[k] for k in names)


class HostBatch(object):
    """Output of the entropy stage: descriptors + the pinned buffer holding [descriptor table | coefficients].  It OWNS one of
    the decoder's two staging buffers until it is passed to reconstruct() (which may be repeated until a later batch takes the
    buffer) or release()d; see JpegDecoder.entropy_decode."""
    __slots__ = ('n', 'descs', 'sizes', 'stage', 'slot', 'gen', 'table_bytes', 'total_bytes', 'entropy', 'scan_off', 'plan_bytes',
                 'scan_bytes', 'coef_bytes', 'status')


class JpegDecoder(ImreadMixin):
    def __init__(self, device='cuda', threads=None, apply_orientation=True, max_pixels=1 << 28, entropy='host', subseq_bytes=None,
                 accept='baseline'):
        """entropy: 'host' (Huffman decoding on the thread pool) or 'device' (on the GPU; the pool runs the marker pass alone).
        subseq_bytes: device mode, bytes of compressed data per lane, a power of two in [8, 4096]; default 32 (8 and 16 decode faster in isolation: profiles/jpeg_bench_device_entropy.txt).
        threads: workers of the entropy stage, default min(16, images of the call); never more than 16, never derived from
        the machine's CPU count.  apply_orientation=False delivers the stored raster (cv2.IMREAD_IGNORE_ORIENTATION).
        max_pixels: a header that claims more is refused before any buffer is sized from it (a few bytes can claim 65535 x 65535).
        accept: 'baseline' (one interleaved scan, 4:4:4 / 4:2:2 / 4:2:0: everything else is refused by name), 'all', or any
        subset of {'progressive', 'multiscan', 'sampling'}: progressive files, sequential files in several scans, and the luma
        factors up to 4 x 4 with at most 8 luma blocks per MCU (4:4:0, 4:1:1, 4:1:0, ...).  Host entropy stage only."""
        self.accept = _accept_mask(accept)
        if entropy == 'device' and self.accept:
            raise PPYoloHipError("the device entropy stage reads single-scan baseline files only: entropy='device' needs "
                                 "accept='baseline', got %r" % (accept,))
        self.max_pixels = int(max_pixels)
        if entropy not in ('host', 'device'):
            raise PPYoloHipError("entropy must be 'host' or 'device', got %r" % (entropy,))
        self.entropy = entropy
        self.subseq_bytes = _lib.JPEG_SUBSEQ_DEFAULT if subseq_bytes is None else int(subseq_bytes)
        if not (_lib.JPEG_SUBSEQ_MIN <= self.subseq_bytes <= _lib.JPEG_SUBSEQ_MAX) or self.subseq_bytes & (self.subseq_bytes - 1):
            raise PPYoloHipError('subseq_bytes must be a power of two in [%d, %d]' % (_lib.JPEG_SUBSEQ_MIN, _lib.JPEG_SUBSEQ_MAX))
        self.last_status = None         # device mode: the status tensor of the last reconstruct()
        self.device = torch.device(device)
        self._host = HostPool(threads, 'ppy-jpeg')
        self.threads = self._host.threads
        self.apply_orientation = bool(apply_orientation)
        self._ring = StagingRing(self.device, 1 << 20, stage='entropy')     # entropy_decode and reconstruct may run on two threads

    # ---- host stage ---------------------------------------------------------------------------------------------------
    _pool = property(lambda self: self._host.executor)      # None until a call needs more than one worker

    def _staging(self, nbytes):
        return self._ring.take(nbytes)

    def release(self, hb):
        """Give back the staging buffer of a HostBatch that will not be reconstructed."""
        self._ring.release(hb.slot, hb.gen)

    def refusal(self, item):
        """Header pass only, nothing is decoded: None if decode() would take the item as far as its markers tell, otherwise
        (kind, reason) with kind 'unsupported' (progressive, arithmetic, ...: a file for another decoder) or 'corrupt'.
        Damage inside the entropy data still surfaces in decode()."""
        data = read_bytes(item)
        info = _lib.JpegInfo()
        rc = lib().ppy_jpeg_info_ex(data, len(data), self.accept, ctypes.byref(info))
        if rc == _lib.OK:
            return None
        return ('unsupported' if rc == -2 else 'corrupt'), info.reason.decode(errors='replace') or '?'

    def entropy_decode(self, items):
        """Host only: parse and Huffman-decode every item into a pinned staging buffer.  The returned HostBatch owns that buffer
        until reconstruct(hb) or release(hb); there are two buffers, so at most two batches can wait at a time (a third call
        raises instead of overwriting one).  May run on another thread than reconstruct()."""
        L = lib()
        datas = [read_bytes(it) for it in items]
        n = len(datas)
        if n == 0:
            raise PPYoloHipError('empty batch')
        if self.entropy == 'device':
            return self._scan_prepare(datas)
        descs = (_lib.JpegDesc * n)()
        sizes = []
        table_bytes = L.ppy_jpeg_table_bytes(n)
        total = table_bytes
        for i, d in enumerate(datas):
            info = _lib.JpegInfo()
            rc = L.ppy_jpeg_info_ex(d, len(d), self.accept, ctypes.byref(info))
            if rc != _lib.OK:
                raise _refuse(i, rc, info.reason)
            if info.width * info.height > self.max_pixels:
                raise PPYoloHipError('item %d: %d x %d pixels is over max_pixels = %d' % (i, info.width, info.height, self.max_pixels))
            descs[i].coef_base = total - table_bytes
            total += (info.coef_bytes + 15) // 16 * 16
            sizes.append((info.height, info.width, info.out_height, info.out_width, info.coef_bytes))
        slot, gen, stage = self._staging(total)
        hb = HostBatch()
        hb.n, hb.descs, hb.sizes, hb.stage, hb.slot, hb.gen, hb.table_bytes, hb.total_bytes = n, descs, sizes, stage, slot, gen, table_bytes, total
        hb.entropy, hb.status = 'host', None
        base = stage.data_ptr() + table_bytes

        def one(i):
            reason = ctypes.create_string_buffer(64)
            rc = L.ppy_jpeg_entropy_decode_ex(datas[i], len(datas[i]), self.accept, base + descs[i].coef_base, sizes[i][4], ctypes.byref(descs[i]),
                                              reason)
            return rc, reason.value

        try:
            for i, (rc, reason) in enumerate(self._host.map(one, n)):
                if rc != _lib.OK:
                    raise _refuse(i, rc, reason)
        except BaseException:
            self.release(hb)
            raise
        return hb

    def _scan_prepare(self, datas):
        """entropy_decode() of the device mode: the marker pass of every item writes its scan record into the staging buffer,
        laid out [descriptor table | plan | records]; the coefficients only ever exist on the device."""
        L = lib()
        n = len(datas)
        descs = (_lib.JpegDesc * n)()
        sizes, scan_off, bounds = [], [], []
        coef_bytes = scan_bytes = segments = 0

        def size(i):          # the two header-only calls that size the buffers, on the pool like the pass itself
            info, segs = _lib.JpegInfo(), ctypes.c_longlong()
            rc = L.ppy_jpeg_info(datas[i], len(datas[i]), ctypes.byref(info))
            bound = L.ppy_jpeg_scan_bytes(datas[i], len(datas[i]), ctypes.byref(segs)) if rc == _lib.OK else 0
            return rc, info, bound, segs

        for i, (rc, info, bound, segs) in enumerate(self._host.map(size, n)):
            d = datas[i]
            if rc != _lib.OK:
                raise _refuse(i, rc, info.reason)
            if info.width * info.height > self.max_pixels:
                raise PPYoloHipError('item %d: %d x %d pixels is over max_pixels = %d' % (i, info.width, info.height, self.max_pixels))
            if bound == 0:
                raise PPYoloHipError('item %d: file of %d bytes is too large for the device entropy stage' % (i, len(d)))
            descs[i].coef_base = coef_bytes
            coef_bytes += (info.coef_bytes + 15) // 16 * 16
            scan_off.append(scan_bytes)
            bounds.append(bound)
            scan_bytes += bound
            segments += segs.value
            sizes.append((info.height, info.width, info.out_height, info.out_width, info.coef_bytes))
        table_bytes = L.ppy_jpeg_table_bytes(n)
        plan_bytes = L.ppy_jpeg_entropy_plan_bytes(n, segments)
        total = table_bytes + plan_bytes + scan_bytes
        slot, gen, stage = self._staging(total)
        hb = HostBatch()
        hb.n, hb.descs, hb.sizes, hb.stage, hb.slot, hb.gen, hb.table_bytes, hb.total_bytes = n, descs, sizes, stage, slot, gen, table_bytes, total
        hb.entropy, hb.status, hb.scan_off, hb.plan_bytes, hb.scan_bytes, hb.coef_bytes = 'device', None, scan_off, plan_bytes, scan_bytes, coef_bytes
        base = stage.data_ptr() + table_bytes + plan_bytes

        def one(i):
            reason = ctypes.create_string_buffer(64)
            rc = L.ppy_jpeg_scan_prepare(datas[i], len(datas[i]), base + scan_off[i], bounds[i], None, ctypes.byref(descs[i]), reason)
            return rc, reason.value

        try:
            for i, (rc, reason) in enumerate(self._host.map(one, n)):
                if rc != _lib.OK:
                    raise _refuse(i, rc, reason)
        except BaseException:
            self.release(hb)
            raise
        return hb

    # ---- device stage -------------------------------------------------------------------------------------------------
    def reconstruct(self, hb, out=None, check=True):
        """Copy a HostBatch to the device and enqueue the two reconstruction launches on the current stream.  out: optional
        list of uint8 device tensors [h,w,3] to fill (pixel stride 3, any row stride).
        A batch of the device entropy mode: the copy carries the compressed data, the entropy launches come before the two
        reconstruction launches, and with check=True (the default) the n status words are read back in one small copy, which
        synchronises the stream once: damage raises PPYoloHipError naming the item, as the host mode does in entropy_decode().
        check=False reads nothing back; hb.status (and self.last_status) is the int32 device tensor [3, n] of status codes,
        reason ids (ppy_jpeg_reason_string) and cross-workgroup repair counts, for the caller to examine later."""
        L = lib()
        n = hb.n
        ori = self.apply_orientation
        shapes = [(s[2], s[3]) if ori else (s[0], s[1]) for s in hb.sizes]
        if out is None:
            out = [torch.empty((h, w, 3), dtype=torch.uint8, device=self.device) for h, w in shapes]
        else:
            check_outputs(out, shapes, self.device)
        device_entropy = hb.entropy == 'device'
        with self._ring.uploading(hb.slot, hb.gen) as staging:
            _check(L.ppy_jpeg_pack_table(n, hb.descs, (ctypes.c_void_p * n)(*[t.data_ptr() for t in out]),
                                         (ctypes.c_longlong * n)(*[row_pitch(t) for t in out]), int(ori),
                                         hb.stage.data_ptr(), hb.table_bytes), 'ppy_jpeg_pack_table')
            if device_entropy:
                h_plan = hb.stage.data_ptr() + hb.table_bytes
                ent_ws = ctypes.c_size_t()
                _check(L.ppy_jpeg_entropy_plan(n, hb.descs, h_plan + hb.plan_bytes, hb.scan_bytes, (ctypes.c_longlong * n)(*hb.scan_off),
                                               self.subseq_bytes, h_plan, hb.plan_bytes, ctypes.byref(ent_ws)), 'ppy_jpeg_entropy_plan')
            blob = staging.copy(hb.total_bytes)
            stream = torch.cuda.current_stream().cuda_stream
            if device_entropy:      # enqueued before the staging buffer is given back: the call sizes its grids from the host plan
                coef = torch.empty(max(hb.coef_bytes, 16), dtype=torch.uint8, device=self.device)
                coef_ptr, coef_bytes = coef.data_ptr(), hb.coef_bytes
                status = torch.empty((3, n), dtype=torch.int32, device=self.device)
                ent = torch.empty(max(ent_ws.value, 16), dtype=torch.uint8, device=self.device)
                _check(L.ppy_jpeg_entropy_device(n, h_plan, blob.data_ptr() + hb.table_bytes, blob.data_ptr() + hb.table_bytes + hb.plan_bytes,
                                                 self.subseq_bytes, coef_ptr, coef_bytes, status.data_ptr(), ent.data_ptr(), ent_ws.value, stream),
                       'ppy_jpeg_entropy_device')
                hb.status = self.last_status = status
            else:
                coef_ptr, coef_bytes = blob.data_ptr() + hb.table_bytes, hb.total_bytes - hb.table_bytes
        ws_bytes = L.ppy_jpeg_workspace_bytes(n, hb.descs)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
        _check(L.ppy_jpeg_reconstruct_u8(n, hb.descs, int(ori), blob.data_ptr(), coef_ptr, coef_bytes, ws.data_ptr(), ws_bytes, stream),
               'ppy_jpeg_reconstruct_u8')
        if device_entropy and check:
            st = status.cpu()          # one small copy; it waits for the stream
            for i in range(n):
                if int(st[0, i]) != _lib.OK:
                    raise _refuse(i, int(st[0, i]), L.ppy_jpeg_reason_string(int(st[1, i])))
        return out

    # ---- the user's calls ---------------------------------------------------------------------------------------------
    def decode(self, items, out=None, check=True):
        """list of bytes / memoryview / paths -> list of uint8 [h,w,3] BGR device tensors, asynchronous on the current stream
        (the device entropy mode with check=True waits for its status words: reconstruct())."""
        hb = self.entropy_decode(items)
        try:
            return self.reconstruct(hb, out=out, check=check)
        except BaseException:
            self.release(hb)        # (outputs refused: the batch never reached the device; after the copy this changes nothing)
            raise


# ---- encoding ---------------------------------------------------------------------------------------------------------------
SUBSAMPLINGS = {'4:4:4': (1, 1), '4:2:2': (2, 1), '4:2:0': (2, 2)}


class EncBatch(object):
    """Output of stage 1: the descriptors, the device table and the device coefficient buffer (the decoder's layout; image i
    at descs[i].coef_base), plus the source tensors, which the kernels read in place and which therefore stay referenced."""
    __slots__ = ('n', 'descs', 'sizes', 'table', 'coef', 'sources')

    def coefficients(self, i):
        """Image i's coefficients as the seam stores them: one int16 device tensor [block rows, block columns, 64] per
        component, whole-MCU block counts, TRANSPOSED inside a block (index column * 8 + row)."""
        d = self.descs[i]
        flat = self.coef[d.coef_base:d.coef_base + d.coef_bytes].view(torch.int16)
        return [flat[d.coef_offset[c]:d.coef_offset[c] + d.blocks_w[c] * d.blocks_h[c] * 64].view(d.blocks_h[c], d.blocks_w[c], 64)
                for c in range(d.components)]


class JpegEncoder(object):
    def __init__(self, quality=95, subsampling='4:2:0', restart_interval=0, entropy='device', device='cuda'):
        """quality: 1..100 (95 is cv2's default; Pillow's is 75).  subsampling: '4:4:4', '4:2:2' or '4:2:0' (libjpeg's and cv2's
        default); a grey image ignores it.  restart_interval: MCUs between restart markers, 0 = none.  entropy: 'device' (the
        bit-packer on the GPU) or 'host' (its host twin: the coefficients are read back instead of the bytes)."""
        if isinstance(quality, bool) or not isinstance(quality, int) or not 1 <= quality <= 100:
            raise PPYoloHipError('quality must be an integer in 1..100, got %r' % (quality,))
        if subsampling not in SUBSAMPLINGS:
            raise PPYoloHipError("subsampling must be one of '4:4:4', '4:2:2', '4:2:0', got %r" % (subsampling,))
        if isinstance(restart_interval, bool) or not isinstance(restart_interval, int) or not 0 <= restart_interval <= 65535:
            raise PPYoloHipError('restart_interval must be an integer in 0..65535 MCUs, got %r' % (restart_interval,))
        if entropy not in ('host', 'device'):
            raise PPYoloHipError("entropy must be 'host' or 'device', got %r" % (entropy,))
        self.quality, self.subsampling, self.restart_interval, self.entropy = quality, subsampling, restart_interval, entropy
        self.device = torch.device(device)
        h, v = SUBSAMPLINGS[subsampling]
        self.params = _lib.JpegEncParams(quality, h, v, restart_interval)
        self._staging = Staging(self.device, 1 << 16)       # the descriptor table is packed into it

    # ---- the parts --------------------------------------------------------------------------------------------------------
    def quant_tables(self):
        """(luma, chroma): the quantiser tables of this quality, 64 ints each in natural (row-major) order."""
        a, b = (ctypes.c_ushort * 64)(), (ctypes.c_ushort * 64)()
        _check(lib().ppy_jpeg_enc_quant(self.quality, a, b), 'ppy_jpeg_enc_quant')
        return list(a), list(b)

    def header(self, width, height, components=3):
        """The bytes from SOI through SOS of a width x height file with 3 (YCbCr) or 1 (grey) components."""
        L = lib()
        cap = L.ppy_jpeg_enc_header_bytes(components, self.restart_interval)
        buf, used, reason = ctypes.create_string_buffer(max(cap, 1)), ctypes.c_size_t(), ctypes.create_string_buffer(64)
        rc = L.ppy_jpeg_enc_header(ctypes.byref(self.params), width, height, components, buf, cap, ctypes.byref(used), reason)
        if rc != _lib.OK:
            raise PPYoloHipError('cannot write a JPEG header: %s (code %d)' % (reason.value.decode() or L.ppy_error_string(rc).decode(), rc))
        return buf.raw[:used.value]

    def _source(self, i, im):
        """One input -> a device tensor the kernels read in place (hostio.check_image, [h,w] grey included, sides in 1..65535);
        numpy arrays and CPU tensors of those shapes are uploaded."""
        if isinstance(im, np.ndarray):
            if im.dtype != np.uint8:
                raise PPYoloHipError('image %d: dtype %s, expected uint8' % (i, im.dtype))
            im = torch.from_numpy(np.ascontiguousarray(im))
        check_image(i, im, self.device, 'source', grey=True, bound=True, host=True)
        return im.contiguous().to(self.device, non_blocking=False) if im.device.type == 'cpu' else im

    def coefficients(self, images):
        """Stage 1: colour conversion, padding, downsampling, forward DCT and quantisation of the whole batch in one launch on
        the current stream -> EncBatch."""
        L = lib()
        srcs = [self._source(i, im) for i, im in enumerate(images)]
        n = len(srcs)
        if n == 0:
            raise PPYoloHipError('empty batch')
        descs = (_lib.JpegEncDesc * n)()
        for d, t in zip(descs, srcs):
            pix = 3 if t.dim() == 3 else 1
            d.src, d.row_stride = t.data_ptr(), max(t.stride(0), pix * t.shape[1])
            d.width, d.height, d.components = t.shape[1], t.shape[0], pix
        sizes, reason = _lib.JpegEncSizes(), ctypes.create_string_buffer(64)
        rc = L.ppy_jpeg_enc_layout(ctypes.byref(self.params), n, descs, ctypes.byref(sizes), reason)
        if rc != _lib.OK:
            raise PPYoloHipError('cannot encode: %s (code %d)' % (reason.value.decode() or L.ppy_error_string(rc).decode(), rc))
        stage = self._staging.acquire(sizes.table_bytes)
        _check(L.ppy_jpeg_enc_pack_table(ctypes.byref(self.params), n, descs, stage.data_ptr(), sizes.table_bytes), 'ppy_jpeg_enc_pack_table')
        eb = EncBatch()
        eb.n, eb.descs, eb.sizes, eb.sources = n, descs, sizes, srcs
        eb.table = self._staging.upload(sizes.table_bytes)
        eb.coef = torch.empty(max(sizes.coef_bytes, 16), dtype=torch.uint8, device=self.device)
        _check(L.ppy_jpeg_enc_coefficients(n, descs, eb.table.data_ptr(), eb.coef.data_ptr(), sizes.coef_bytes,
                                           torch.cuda.current_stream().cuda_stream), 'ppy_jpeg_enc_coefficients')
        return eb

    def scan_device(self, eb):
        """Stage 2 on the device: eight launches on the current stream, nothing read back -> (out, lengths): a uint8 device
        tensor holding the images' entropy-coded bytes back to back, and their sizes (int64 device tensor [n])."""
        L = lib()
        ws = torch.empty(max(eb.sizes.ws_bytes, 16), dtype=torch.uint8, device=self.device)
        out = torch.empty(max(eb.sizes.out_bytes, 16), dtype=torch.uint8, device=self.device)
        lengths = torch.empty(eb.n, dtype=torch.int64, device=self.device)
        rc = L.ppy_jpeg_enc_scan_device(eb.n, eb.descs, eb.table.data_ptr(), eb.coef.data_ptr(), eb.sizes.coef_bytes, out.data_ptr(),
                                        eb.sizes.out_bytes, lengths.data_ptr(), ws.data_ptr(), eb.sizes.ws_bytes,
                                        torch.cuda.current_stream().cuda_stream)
        if rc == _lib.ERR_UNSUPPORTED:
            raise PPYoloHipError("an image of the batch is too large for the device entropy stage (its capacity bound is over 2^29 "
                                 "bytes): use JpegEncoder(entropy='host')")
        _check(rc, 'ppy_jpeg_enc_scan_device')
        return out, lengths

    def scan_host(self, eb, coef=None):
        """Stage 2 through the host twin -> list of entropy-coded byte strings.  coef: the host copy of the batch's
        coefficient buffer (a uint8 CPU tensor); default: eb.coef read back, which waits for the stream."""
        L = lib()
        coef = eb.coef.cpu() if coef is None else coef
        scans = []
        for i in range(eb.n):
            d = eb.descs[i]
            buf, used, reason = ctypes.create_string_buffer(d.scan_capacity), ctypes.c_size_t(), ctypes.create_string_buffer(64)
            rc = L.ppy_jpeg_enc_scan_host(ctypes.byref(d), coef.data_ptr() + d.coef_base, d.coef_bytes, buf, d.scan_capacity,
                                          ctypes.byref(used), reason)
            if rc != _lib.OK:
                raise PPYoloHipError('image %d: %s (code %d)' % (i, reason.value.decode() or L.ppy_error_string(rc).decode(), rc))
            scans.append(buf.raw[:used.value])
        return scans

    # ---- the user's calls -------------------------------------------------------------------------------------------------
    def encode(self, images):
        """list of images -> list of bytes, each a complete JPEG file.  Asynchronous on the current stream up to the read-back:
        two blocking copies, one stream wait -- the lengths (this waits for the stream), then exactly that many bytes, which
        finds the stream idle.  A numpy or CPU-tensor input adds one blocking upload each; device tensors add none."""
        eb = self.coefficients(images)
        if self.entropy == 'device':
            out, lengths = self.scan_device(eb)
            lens = lengths.cpu().tolist()
            data = out[:sum(lens)].cpu().numpy().tobytes()
            scans, off = [], 0
            for ln in lens:
                scans.append(data[off:off + ln])
                off += ln
        else:
            scans = self.scan_host(eb)
        return [self.header(d.width, d.height, d.components) + s + b'\xff\xd9' for d, s in zip(eb.descs, scans)]

    def imencode(self, img):
        return self.encode([img])[0]

    def imwrite(self, path, img):
        data = self.imencode(img)
        with open(path, 'wb') as fh:
            fh.write(data)
