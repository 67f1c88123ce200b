"""Pillow's `Image.resize` on the device, bit for bit (csrc/pil_resize.hip).

    from ppyolo_hip.resize import PilResizer, BICUBIC
    thumbs = PilResizer(BICUBIC)(images, size=(160, 120))      # list of uint8 [120, 160, 3] device tensors

The coefficient tables are planned in the library (ppy_pil_resize_plan, C++ on the host: nothing per image is built in the
interpreter), one per distinct axis of the batch, and cross to the device in one copy out of a pinned buffer this object owns;
the intermediate images of the two-pass filters live in a device workspace it owns too.  Both grow on demand."""
import numpy as np
import torch

from . import _lib, ops
from ._lib import PPYoloHipError
from .hostio import Staging, check_image, row_pitch

NEAREST, LANCZOS, BILINEAR, BICUBIC, BOX, HAMMING = range(6)      # Pillow's codes, the ones the reference's `interp` carries


def check_filter(filter, what='filter'):
    if isinstance(filter, bool) or not isinstance(filter, (int, np.integer)) or int(filter) not in _lib.PIL_FILTERS:
        raise PPYoloHipError('%s=%r: expected one of Pillow\'s filter codes %s' % (
            what, filter, ', '.join('%d %s' % kv for kv in sorted(_lib.PIL_FILTERS.items()))))
    return int(filter)


class PilPlanner(object):
    """The host half of a launch, shared by PilResizer and Preprocessor: plans a batch into the pinned staging buffer, copies the
    blob to the device and sizes the workspace.  One staging buffer: planning the next batch first waits on the host for the
    copy of the batch before it (not for its launches; hostio.Staging)."""

    def __init__(self, filter, device):
        self.filter = check_filter(filter)
        self.device = torch.device(device)
        self._staging = Staging(self.device, 1 << 16, factor=2)     # the planner writes into it
        self._ws = None                 # device workspace: the uint8 intermediates
        self._keep = None               # what the launches in flight read

    def plan(self, images, ow, oh):
        """images: uint8 [h,w,3] tensors on self.device with pixel stride 3.  Returns (n, host address of the blob, its device
        copy, blob bytes, workspace or None)."""
        descs = [(t.data_ptr(), row_pitch(t), t.shape[0], t.shape[1]) for t in images]
        nbytes, ws_bytes = ops.pil_resize_plan(descs, ow, oh, self.filter, lambda nb: self._staging.acquire(nb).data_ptr())
        blob = self._staging.upload(nbytes)
        if ws_bytes and (self._ws is None or self._ws.numel() < ws_bytes):
            self._ws = torch.empty(max(ws_bytes, 1 << 20), dtype=torch.uint8, device=self.device)
        cur = torch.cuda.current_stream(self.device)
        for t in list(images) + ([self._ws] if ws_bytes else []):      # memory another stream's decoder or lane may own
            t.record_stream(cur)
        self._keep = (blob, list(images), self._ws)
        return len(images), self._staging.buffer.data_ptr(), blob, nbytes, (self._ws if ws_bytes else None)


def device_source(i, im, device):
    """One source -> a uint8 [h,w,3] tensor on `device` the kernels read where it lies (hostio.check_image); a numpy array is
    uploaded; anything else raises with the reason."""
    if isinstance(im, np.ndarray):
        if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
            raise PPYoloHipError('image %d: numpy %s %s, expected uint8 [h, w, 3]' % (i, im.dtype, tuple(im.shape)))
        return torch.from_numpy(np.ascontiguousarray(im)).to(device, non_blocking=False)
    return check_image(i, im, device, 'source')


def check_boxes(shapes, box):
    """Pillow's own test of `resize(box=)`, on the host: shapes = [(h, w)], box = one (x0, y0, x1, y1) per image -> float32
    [n, 4], rounded as Pillow's "(ffff)" rounds them.  A box Pillow refuses raises, naming the image and the value."""
    try:
        b = np.array([[float(v) for v in one] for one in box], dtype=np.float64)
    except (TypeError, ValueError):
        raise PPYoloHipError('box=%r: expected one (x0, y0, x1, y1) per image' % (box,))
    if b.shape != (len(shapes), 4):
        raise PPYoloHipError('box: an array of shape %s for %d images, expected one (x0, y0, x1, y1) per image'
                             % (b.shape, len(shapes)))
    with np.errstate(over='ignore'):
        b = b.astype(np.float32)
    for i, ((h, w), (x0, y0, x1, y1)) in enumerate(zip(shapes, b)):
        if not np.isfinite(b[i]).all():
            raise PPYoloHipError('image %d: box %s is not finite' % (i, tuple(b[i].tolist())))
        if x0 < 0 or y0 < 0:                # Pillow: "box offset can't be negative"
            raise PPYoloHipError('image %d: box offset can\'t be negative: (x0, y0) = (%r, %r)' % (i, float(x0), float(y0)))
        if x1 > w or y1 > h:                # Pillow: "box can't exceed original image size"
            raise PPYoloHipError('image %d: box can\'t exceed original image size %d x %d: (x1, y1) = (%r, %r)'
                                 % (i, w, h, float(x1), float(y1)))
        if not (x0 < x1 and y0 < y1):       # (Pillow refuses x1 < x0 and resizes an empty box to a constant; the kernels skip both)
            raise PPYoloHipError('image %d: box (%r, %r, %r, %r) is empty' % (i, float(x0), float(y0), float(x1), float(y1)))
    return b


class PilResizer(object):
    """`Image.fromarray(im).resize(size, filter)` for a batch of 3-channel uint8 images of any sizes, on the device."""

    def __init__(self, filter, device='cuda'):
        self.device = torch.device(device)
        self._planner = PilPlanner(filter, self.device)
        self.filter = self._planner.filter
        self._cropper = None            # the launcher of the box= path (ppyolo_hip/crops.py), made on first use

    def __call__(self, images, size, box=None):
        """images: list of uint8 [h,w,3] device tensors (read in place) or numpy arrays (uploaded); size = (ow, oh), Pillow's
        order.  Returns a list of uint8 [oh, ow, 3] device tensors (views of one batch tensor), asynchronous on the current
        stream: two launches, or one when no image changes its width.
        box: None, or one (x0, y0, x1, y1) per image, Pillow's `resize(size, filter, box=)`: the values are rounded to float32
        as Pillow's C does and run through the crop kernels (csrc/pil_crop.hip; four launches).  A box
        Pillow refuses raises PPYoloHipError naming the image and the value, on the host."""
        if box is not None:
            return self._call_box(list(images), size, box)
        images = list(images)
        if not images:
            raise PPYoloHipError('empty batch')
        try:
            ow, oh = (int(v) for v in size)
        except (TypeError, ValueError):
            raise PPYoloHipError('size=%r: expected (width, height)' % (size,))
        dev = [device_source(i, im, self.device) for i, im in enumerate(images)]
        if ow < 1 or oh < 1:        # (the planner refuses the rest by name; an empty tensor cannot be allocated before it)
            raise PPYoloHipError('output size %d x %d, each side must be in 1..8192' % (ow, oh))
        n, h_blob, blob, nbytes, ws = self._planner.plan(dev, ow, oh)
        out = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device=self.device)
        ops.pil_resize_u8(n, h_blob, blob, nbytes, ws, out)
        return list(out.unbind(0))

    def _call_box(self, images, size, box):
        from . import crops
        if self._cropper is None:
            self._cropper = crops.CropLauncher(self.filter, self.device)
        ow, oh = crops.check_size(size)
        dev = self._cropper.sources(images)
        b = check_boxes([(t.shape[0], t.shape[1]) for t in dev], box)
        n = len(dev)
        descs, d_images, ws, out, src, total, boxes = self._cropper.prepare(dev, 1, n, ow, oh)
        d_boxes = torch.from_numpy(b).to(self.device)
        d_index = torch.arange(n, dtype=torch.int32, device=self.device)
        ops.pil_crop_list_u8(descs, n, d_images, d_boxes, d_index, ow, oh, self.filter, ws, out, src, total, boxes)
        return list(out.unbind(0))          # (every box passed the kernels' own test above: crop i is image i)


def parse_plan(blob):
    """A planner blob (numpy uint8) -> dict(header fields, images = list of dicts, tables = {byte offset: dict(in, out, ksize,
    kind, bounds int32 [out, 2], k int32 [out, ksize])}): the layout include/ppyolo_hip.h documents, for tests and tools."""
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    hi = blob[:32].view(np.int32)
    hl = blob[32:48].view(np.int64)
    ho = blob[48:56].view(np.int32)
    hd = dict(magic=bytes(blob[:4]), n=int(hi[1]), ow=int(hi[2]), oh=int(hi[3]), filter=int(hi[4]), n_tables=int(hi[5]),
              max_h_horizontal=int(hi[6]), mid_pitch=int(hi[7]), blob_bytes=int(hl[0]), ws_bytes=int(hl[1]),
              desc_offset=int(ho[0]), table_offset=int(ho[1]), images=[], tables={})
    for i in range(hd['n']):
        rec = blob[hd['desc_offset'] + 48 * i:hd['desc_offset'] + 48 * (i + 1)]
        q, d = rec.view(np.int64), rec.view(np.int32)
        hd['images'].append(dict(base=int(q[0]), pitch=int(q[1]), h=int(d[4]), w=int(d[5]), xtab=int(d[6]), ytab=int(d[7]),
                                 mid_offset=int(q[4])))
    for im in hd['images']:
        for off in (im['xtab'], im['ytab']):
            if off < 0 or off in hd['tables']:
                continue
            t = blob[off:off + 16].view(np.int32)
            insz, outsz, ksize, kind = (int(v) for v in t)
            b0 = off + 16
            bounds = blob[b0:b0 + 8 * outsz].view(np.int32).reshape(outsz, 2).copy()
            k = blob[b0 + 8 * outsz:b0 + 8 * outsz + 4 * outsz * ksize].view(np.int32).reshape(outsz, ksize).copy()
            hd['tables'][off] = dict(insz=insz, outsz=outsz, ksize=ksize, kind=kind, bounds=bounds, k=k)
    return hd


def plan_host(sizes, ow, oh, filter):
    """The planner alone, without a device: sizes = list of (h, w) -> (numpy blob, workspace bytes).  The descriptors carry a
    placeholder address; the blob is for inspection (parse_plan), not for a launch."""
    hold = []

    def alloc(nbytes):
        hold.append(np.zeros((nbytes + 7) // 8, np.int64))
        return hold[-1].ctypes.data

    nbytes, ws_bytes = ops.pil_resize_plan([(8, 3 * w, h, w) for h, w in sizes], ow, oh, check_filter(filter), alloc)
    return hold[-1].view(np.uint8)[:nbytes], ws_bytes
