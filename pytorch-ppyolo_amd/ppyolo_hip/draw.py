"""Boxes and labels on uint8 device images: the reference's Decode.draw (model/decode_np.py:98-123) as one launch per batch
(csrc/draw.hip), between JpegDecoder / the network and JpegEncoder, so an annotated file never visits the host as pixels.

What is the reference's: which rows are drawn and in which order, the rounding of the corners, the colour of each class, the
label string '%s: %.2f', where the label's background and text sit.  What is NOT: the glyphs.  cv2.putText's anti-aliased
Hershey font cannot be pinned without cv2; the text here is Pillow's built-in bitmap font (ppyolo_hip/label_font.py, 6 x 11
cells), so the output equals Pillow's ImageDraw applied in the same order, bit for bit (tests/draw_ref.py), and differs from
cv2's inside the label.  Pillow is not imported at run time.  DESIGN.md section 10c."""
import colorsys
import ctypes
import random

import torch

from . import _lib, label_font, ops
from ._lib import PPYoloHipError
from .hostio import Staging, check_image, row_pitch, same_device


def class_colors(num_classes):
    """Reference model/decode_np.py:101-107: the hsv wheel, int(v * 255), shuffled with seed 0 -- by a generator of its own,
    which gives the order random.seed(0); random.shuffle gives and leaves the global generator alone."""
    colors = [colorsys.hsv_to_rgb(1.0 * x / num_classes, 1., 1.) for x in range(num_classes)]
    colors = [(int(c[0] * 255), int(c[1] * 255), int(c[2] * 255)) for c in colors]
    random.Random(0).shuffle(colors)
    return colors


def label_codes(name):
    """A class name as the character codes the kernel draws: anything outside 32..126 becomes '?'."""
    return [ord(c) if label_font.FIRST <= ord(c) <= label_font.LAST else ord('?') for c in name]


class BoxDrawer(object):
    def __init__(self, all_classes, device='cuda'):
        """all_classes: the class names in class-index order (at most 64 characters each).  The colour table, the names and the
        font are built here once and uploaded once, with the first draw."""
        self.all_classes = [str(c) for c in all_classes]
        self.num_classes = len(self.all_classes)
        if self.num_classes < 1:
            raise PPYoloHipError('BoxDrawer needs at least one class name')
        for i, name in enumerate(self.all_classes):
            if len(name) > _lib.DRAW_NAME_MAX:
                raise PPYoloHipError('class %d: name of %d characters, at most %d are drawn' % (i, len(name), _lib.DRAW_NAME_MAX))
        self.device = torch.device(device)
        self.colors = class_colors(self.num_classes)
        self._h_name_len = (ctypes.c_int * self.num_classes)(*[len(n) for n in self.all_classes])
        self._tables = None             # (colors, names, name_len, font) on the device
        self._staging = Staging(self.device, 1 << 12)       # the image table is written into it

    # ---- the parts --------------------------------------------------------------------------------------------------------
    def _upload(self):
        if self._tables is None:
            names = torch.zeros((self.num_classes, _lib.DRAW_NAME_MAX), dtype=torch.uint8)
            for i, name in enumerate(self.all_classes):
                names[i, :len(name)] = torch.tensor(label_codes(name), dtype=torch.uint8)
            font = torch.frombuffer(bytearray(label_font.device_table()), dtype=torch.uint8).view(95, 16)
            host = (torch.tensor(self.colors, dtype=torch.uint8).view(self.num_classes, 3), names,
                    torch.tensor(list(self._h_name_len), dtype=torch.int32), font)
            self._tables = tuple(t.to(self.device) for t in host)
        return self._tables

    def _target(self, i, im):
        """One image -> itself, if the kernel can draw on it where it lies (hostio.check_image, sides in 1..65535).  Host memory
        is refused, not uploaded: the caller would never see the drawing (draw_host is the call for a numpy image)."""
        if not isinstance(im, torch.Tensor):
            raise PPYoloHipError('image %d: expected a uint8 device tensor [h, w, 3], got %s: BoxDrawer draws in place and does not '
                                 'copy a host array (draw_host takes a numpy image)' % (i, type(im).__name__))
        return check_image(i, im, self.device, 'drawing in place', bound=True)

    def _rows(self, n, dets, count):
        for name, t, dtype in (('dets', dets, torch.float32), ('count', count, torch.int32)):
            if not isinstance(t, torch.Tensor):
                raise PPYoloHipError('%s: expected a device tensor as forward_padded returns it, got %s' % (name, type(t).__name__))
            if not same_device(t.device, self.device):
                raise PPYoloHipError('%s lives on %s, the drawer on %s' % (name, t.device, self.device))
            if t.dtype != dtype:
                raise PPYoloHipError('%s: dtype %s, expected %s' % (name, t.dtype, dtype))
        if dets.dim() != 3 or dets.shape[0] != n or dets.shape[2] != 6 or tuple(count.shape) != (n,):
            raise PPYoloHipError('dets %s and count %s for %d images: expected [%d, K, 6] and [%d]'
                                 % (tuple(dets.shape), tuple(count.shape), n, n, n))
        if not 1 <= dets.shape[1] <= _lib.DRAW_MAX_ROWS:
            raise PPYoloHipError('dets: %d rows per image, supported: 1..%d' % (dets.shape[1], _lib.DRAW_MAX_ROWS))
        if not dets.is_contiguous() or not count.is_contiguous():
            raise PPYoloHipError('dets strides %s, count strides %s: both must be contiguous' % (tuple(dets.stride()), tuple(count.stride())))

    # ---- the user's calls -------------------------------------------------------------------------------------------------
    def __call__(self, images, dets, count, draw_thresh=0.0):
        """Draw rows r < count[i] of dets[i] with score >= draw_thresh on images[i], in place, in row order; one launch on the
        current stream, nothing read back.  images: list of uint8 [h,w,3] device tensors (decoder outputs, crops of larger
        tensors, ...); dets [N,K,6] float32 and count [N] int32 as PPYOLO.forward_padded returns them.  Returns `images`.
        The image table crosses in one small copy out of ONE pinned staging buffer, so a second call first waits on the host
        for the copy of the call before it (not for its launch; hostio.Staging): calls queued back to back behind a deep stream
        are paced by that copy."""
        images = list(images)
        n = len(images)
        if n == 0:
            raise PPYoloHipError('empty batch')
        for i, im in enumerate(images):
            self._target(i, im)
        self._rows(n, dets, count)
        colors, names, name_len, font = self._upload()
        descs = (_lib.DrawImage * n)()
        for d, t in zip(descs, images):
            d.base, d.pitch, d.h, d.w = t.data_ptr(), row_pitch(t), t.shape[0], t.shape[1]
        nbytes = ctypes.sizeof(descs)
        ctypes.memmove(self._staging.acquire(nbytes).data_ptr(), descs, nbytes)
        table = self._staging.upload(nbytes)
        cur = torch.cuda.current_stream(self.device)
        for t in images + [dets, count]:        # the launch touches memory another stream's decoder or lane may own
            t.record_stream(cur)
        ops.draw_detections(descs, table, dets, count, draw_thresh, colors, names, name_len, self._h_name_len, font)
        return images

    def draw_host(self, image, boxes, scores, classes):
        """The reference's Decode.draw(image, boxes, scores, classes): a numpy uint8 [h,w,3] image is uploaded, drawn and copied
        back into the caller's array in place (one blocking round trip); every row given is drawn.  Returns `image`."""
        import numpy as np
        if not isinstance(image, np.ndarray):
            raise PPYoloHipError('draw_host: expected a numpy uint8 image [h, w, 3], got %s' % type(image).__name__)
        if image.dtype != np.uint8:
            raise PPYoloHipError('draw_host: dtype %s, expected uint8' % image.dtype)
        if image.ndim != 3 or image.shape[2] != 3:
            raise PPYoloHipError('draw_host: shape %s, expected [h, w, 3]' % (tuple(image.shape),))
        if not image.flags.writeable:
            raise PPYoloHipError('draw_host: the image is read-only; drawing happens in place (pass a copy)')
        scores = np.asarray(scores, np.float32).reshape(-1)
        m = len(scores)
        if m == 0:
            return image
        boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
        classes = np.asarray(classes).reshape(-1)
        if len(boxes) != m or len(classes) != m:
            raise PPYoloHipError('draw_host: %d boxes, %d scores, %d classes' % (len(boxes), m, len(classes)))
        if not (np.isfinite(scores).all() and (scores >= 0).all() and (scores <= 1).all()):
            raise PPYoloHipError('draw_host: a score outside [0, 1]: the label prints d.dd')
        if not np.isfinite(boxes).all():
            raise PPYoloHipError('draw_host: a box coordinate is not finite')
        if not ((classes >= 0).all() and (classes < self.num_classes).all()):
            raise PPYoloHipError('draw_host: a class outside 0..%d' % (self.num_classes - 1))
        rows = np.concatenate([classes.astype(np.float32)[:, None], scores[:, None], boxes], axis=1)
        dev = torch.from_numpy(np.ascontiguousarray(image)).to(self.device)
        for lo in range(0, m, _lib.DRAW_MAX_ROWS):          # in row order on one stream: a later chunk paints over an earlier one
            part = torch.from_numpy(np.ascontiguousarray(rows[lo:lo + _lib.DRAW_MAX_ROWS])[None]).to(self.device)
            cnt = torch.tensor([part.shape[1]], dtype=torch.int32, device=self.device)
            self([dev], part, cnt, 0.0)
        image[...] = dev.cpu().numpy()
        return image
