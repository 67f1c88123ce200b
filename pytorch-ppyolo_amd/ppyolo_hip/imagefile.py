"""One decoder for a folder that holds both formats: ImageDecoder sniffs the first bytes of every item and hands the JPEG files
to a jpeg.JpegDecoder and the PNG files to a png.PngDecoder, each part in ONE decode() call of its decoder.  It has the calls
the `decoder=` hook of Decode.detect_files / annotate_files, TrainBatchBuilder.from_files and augment.decode_records uses
(decode, refusal), plus imread / imdecode, so `decoder=ImageDecoder()` makes all of them read both formats."""
import re

from ._lib import PPYoloHipError
from .hostio import ImreadMixin, read_bytes

PNG_SIGNATURE = b'\x89PNG\r\n\x1a\n'


def sniff(data):
    """'png', 'jpeg' or None from the first 8 bytes."""
    head = bytes(data[:8])
    if head == PNG_SIGNATURE:
        return 'png'
    if head[:2] == b'\xff\xd8':
        return 'jpeg'
    return None


def _neither(data):
    return 'neither a JPEG nor a PNG file (first bytes %s)' % (bytes(data[:8]).hex() or 'missing')


class ImageDecoder(ImreadMixin):
    def __init__(self, jpeg=None, png=None):
        """jpeg / png: the caller's decoders (any object with decode and, optionally, refusal); default: a JpegDecoder() and a
        PngDecoder() of this object's own, made when the first file of the kind arrives."""
        self._dec = {'jpeg': jpeg, 'png': png}

    def _decoder(self, kind):
        if self._dec[kind] is None:
            if kind == 'jpeg':
                from .jpeg import JpegDecoder
                self._dec[kind] = JpegDecoder()
            else:
                from .png import PngDecoder
                self._dec[kind] = PngDecoder()
        return self._dec[kind]

    def refusal(self, item):
        """None, or (kind, reason) as the item's own decoder gives it; an item of neither format is 'unsupported'."""
        data = read_bytes(item)
        kind = sniff(data)
        if kind is None:
            return 'unsupported', _neither(data)
        fn = getattr(self._decoder(kind), 'refusal', None)
        return fn(data) if fn is not None else None

    def decode(self, items, out=None):
        """list of bytes / memoryview / paths of either format -> list of uint8 [h,w,3] BGR device tensors in the caller's
        order.  `item i:` in an error is the caller's index."""
        datas = [read_bytes(it) for it in items]
        if not datas:
            raise PPYoloHipError('empty batch')
        if out is not None and len(out) != len(datas):
            raise PPYoloHipError('%d output tensors for %d images' % (len(out), len(datas)))
        parts = {'jpeg': [], 'png': []}
        for i, d in enumerate(datas):
            kind = sniff(d)
            if kind is None:
                raise PPYoloHipError('item %d: unsupported: %s' % (i, _neither(d)))
            parts[kind].append(i)
        result = [None] * len(datas)
        for kind in ('jpeg', 'png'):
            idx = parts[kind]
            if not idx:
                continue
            try:
                sub = [datas[i] for i in idx]
                ims = self._decoder(kind).decode(sub) if out is None else self._decoder(kind).decode(sub, out=[out[i] for i in idx])
            except PPYoloHipError as e:                 # 'item k: ...' of the part -> the caller's index
                m = re.match(r'item (\d+): (.*)', str(e), re.S)
                if m is None or int(m.group(1)) >= len(idx):
                    raise
                raise PPYoloHipError('item %d: %s' % (idx[int(m.group(1))], m.group(2))) from e
            if len(ims) != len(idx):
                raise PPYoloHipError('the %s decoder returned %d images for %d files' % (kind, len(ims), len(idx)))
            for i, im in zip(idx, ims):
                result[i] = im
        return result
