"""Crops of detections on the device: Pillow's `Image.resize(size, filter, box=...)`, bit for bit, with the boxes read where the
detector left them (csrc/pil_crop.hip).

    from ppyolo_hip.crops import DetectionCropper
    cropper = DetectionCropper(size=(128, 128), pad=0.1)
    dets, count, _ = model.forward_padded(x, im_size)
    crops, src, total = cropper(images, dets, count, thresh=0.3)      # all on the device, nothing waits for the host
    per_image = cropper.split(crops, src, total)                      # [(rows, uint8 [k, 128, 128, 3]), ...]: the one sync

The host knows the image sizes and nothing else: it validates them, sizes the workspace and the grids from them, and copies
the n image descriptors to the device out of a pinned buffer.  Selection, coefficient tables and both passes are kernels."""
import ctypes

import numpy as np
import torch

from . import _lib, ops
from ._lib import PPYoloHipError
from .hostio import Staging, row_pitch
from .resize import BICUBIC, check_filter, device_source

DESC_BYTES = ctypes.sizeof(_lib.PilImage)


class CropLauncher(object):
    """What DetectionCropper and PilResizer(box=) share: the descriptors' staging buffer, the growing device workspace, the
    output tensors and the stream bookkeeping of one call.  One staging buffer: the next call first waits on the host for the
    copy of the descriptors before it (not for its launches; hostio.Staging)."""

    def __init__(self, filter, device):
        self.filter = check_filter(filter)
        self.device = torch.device(device)
        self._staging = Staging(self.device, 1 << 12, factor=2)
        self._ws = None
        self._keep = None               # what the launches in flight read

    def sources(self, images):
        images = list(images)
        if not images:
            raise PPYoloHipError('empty batch')
        return [device_source(i, im, self.device) for i, im in enumerate(images)]

    def prepare(self, dev, form, rows_or_m, ow, oh, pad=0.0, top_k=1):
        """Validates on the host, uploads the descriptors, sizes the workspace.  Returns (host descriptors, their device copy,
        workspace, out, src, total, boxes) with cap = n * K (form 0) or M (form 1)."""
        n = len(dev)
        descs = ops.pil_crop_descs([(t.data_ptr(), row_pitch(t), t.shape[0], t.shape[1]) for t in dev])
        ws_bytes, _ = ops.pil_crop_plan_bytes(descs, n, form, rows_or_m, ow, oh, self.filter, pad, top_k)
        cap = n * rows_or_m if form == 0 else rows_or_m
        buf = self._staging.acquire(n * DESC_BYTES)
        ctypes.memmove(buf.data_ptr(), ctypes.addressof(descs), n * DESC_BYTES)
        d_images = self._staging.upload(n * DESC_BYTES)
        if self._ws is None or self._ws.numel() < ws_bytes:
            self._ws = torch.empty(max(ws_bytes, 1 << 20), dtype=torch.uint8, device=self.device)
        out = torch.empty((cap, oh, ow, 3), dtype=torch.uint8, device=self.device)
        src = torch.empty((cap, 2), dtype=torch.int32, device=self.device)
        total = torch.empty((1,), dtype=torch.int32, device=self.device)
        boxes = torch.empty((cap, 4), dtype=torch.float32, device=self.device)
        cur = torch.cuda.current_stream(self.device)
        for t in list(dev) + [self._ws]:      # memory another stream's decoder or lane may own
            t.record_stream(cur)
        self._keep = (d_images, list(dev), self._ws)
        return descs, d_images, self._ws, out, src, total, boxes


def check_size(size):
    try:
        ow, oh = (int(v) for v in size)
    except (TypeError, ValueError):
        raise PPYoloHipError('size=%r: expected (width, height)' % (size,))
    if ow < 1 or oh < 1:        # (the library refuses the rest by name; an empty tensor cannot be allocated before it)
        raise PPYoloHipError('output size %d x %d, each side must be in 1..8192' % (ow, oh))
    return ow, oh


class DetectionCropper(object):
    """`Image.fromarray(images[i]).resize(size, filter, box=row's box)` for the rows of `forward_padded`, on the device.

    size = (ow, oh), Pillow's order; filter: one of Pillow's codes; pad: every box grows by pad * its width / height on each
    side, clipped to the image; top_k: at most that many crops per image (None: every row that passes)."""

    def __init__(self, size, filter=BICUBIC, pad=0.0, top_k=None, device='cuda'):
        self.ow, self.oh = check_size(size)
        self.device = torch.device(device)
        self._launcher = CropLauncher(filter, self.device)
        self.filter = self._launcher.filter
        try:
            self.pad = float(pad)
        except (TypeError, ValueError):
            raise PPYoloHipError('pad=%r: expected a number in [0, 4]' % (pad,))
        if top_k is not None and (isinstance(top_k, bool) or not isinstance(top_k, (int, np.integer))):
            raise PPYoloHipError('top_k=%r: expected None or an integer >= 1' % (top_k,))
        self.top_k = None if top_k is None else int(top_k)
        self.boxes = None               # float32 [n * K, 4] of the last call: the boxes that were resized (padded, clipped)
        self._n = 0

    def __call__(self, images, dets, count, thresh=0.0):
        """images: n uint8 [h,w,3] device tensors (read in place) or numpy arrays (uploaded); dets float32 [n, K, 6] and count
        int32 [n] on the device, as forward_padded returns them.  Returns (crops uint8 [n * K, oh, ow, 3], zero past total;
        src int32 [n * K, 2] = (image, row) in image-major order, -1 past total; total int32 [1]), all on the device and
        asynchronous on the current stream: four launches."""
        dev = self._launcher.sources(images)
        for name, t, dtype in (('dets', dets, torch.float32), ('count', count, torch.int32)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype:
                raise PPYoloHipError('%s must be a %s device tensor as forward_padded returns it (no CPU path), got %s'
                                     % (name, str(dtype).replace('torch.', ''), 'a %s %s tensor' % (t.device, t.dtype)
                                        if isinstance(t, torch.Tensor) else type(t).__name__))
        n = len(dev)
        if dets.dim() != 3 or dets.shape[0] != n or dets.shape[2] != 6 or tuple(count.shape) != (n,):
            raise PPYoloHipError('dets %s and count %s for %d images: expected [n, K, 6] and [n]'
                                 % (tuple(dets.shape), tuple(count.shape), n))
        K = dets.shape[1]
        if K < 1:
            raise PPYoloHipError('dets %s: no rows per image' % (tuple(dets.shape),))
        thresh = float(thresh)
        if thresh != thresh:
            raise PPYoloHipError('thresh is NaN')
        dets, count = dets.contiguous(), count.contiguous()
        top_k = K if self.top_k is None else self.top_k
        descs, d_images, ws, out, src, total, boxes = self._launcher.prepare(dev, 0, K, self.ow, self.oh, self.pad, top_k)
        ops.pil_crop_rows_u8(descs, d_images, dets, count, thresh, self.pad, top_k, self.ow, self.oh, self.filter, ws, out, src,
                             total, boxes)
        self.boxes, self._n = boxes, n
        return out, src, total

    def split(self, crops, src, total, n=None):
        """The one host synchronisation: reads total and src back and returns, per image, (rows int32 numpy [k], uint8
        [k, oh, ow, 3] device tensor: a view of crops).  n: the number of images (default: of the last call)."""
        n = self._n if n is None else int(n)
        t = int(total.cpu()[0])
        s = src[:t].cpu().numpy()
        res = []
        for i in range(n):
            idx = np.flatnonzero(s[:, 0] == i)
            lo, hi = (int(idx[0]), int(idx[-1]) + 1) if idx.size else (0, 0)
            assert hi - lo == idx.size          # image-major: one run per image
            res.append((s[lo:hi, 1].copy(), crops[lo:hi]))
        return res
