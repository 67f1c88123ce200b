"""The host-side plumbing of the image pipeline (JPEG / PNG decode, JPEG encode, Pillow resize, box drawing, device-resident
training batches), stated once: reading an item's bytes, the device rule, the rule for an image the kernels read or write
where it lies, the pinned staging buffer with its event, the two-buffer ring of the decoders, and their thread pool.  Torch
only: nothing here calls the library, so all of it runs without a GPU."""
import contextlib
import os
import threading
from concurrent.futures import ThreadPoolExecutor

import torch

from ._lib import PPYoloHipError

MAX_THREADS = 16


def read_bytes(item):
    if isinstance(item, (bytes, bytearray, memoryview)):
        return bytes(item)
    if isinstance(item, (str, os.PathLike)):
        with open(item, 'rb') as fh:
            return fh.read()
    raise PPYoloHipError('expected bytes, a memoryview or a path, got %s' % type(item).__name__)


def same_device(a, b):
    """An unindexed 'cuda' means the current device.  The runtime is asked only when both sides are cuda and exactly one index
    is missing: CPU-only use never touches it."""
    a = a if type(a) is torch.device else torch.device(a)
    b = b if type(b) is torch.device else torch.device(b)
    if a == b:
        return True
    kind, ai, bi = a.type, a.index, b.index
    if kind != b.type or (ai is not None and bi is not None):
        return False
    return kind != 'cuda' or torch.cuda.current_device() == (bi if ai is None else ai)


# ---- images the kernels read or write where they lie ----------------------------------------------------------------------------
def row_pitch(t):
    """Bytes from one row of an in-place image to the next (a one-row image may carry any row stride, 0 included)."""
    return max(t.stride(0), 3 * t.shape[1])


# noun -> (what the item is called, the subject of the stride sentence, what the caller can do about it)
_NOUNS = {'source': ('image', 'a source', '; call `.contiguous()` on it first'),
          'output': ('output', 'an output', ''),
          'drawing in place': ('image', 'drawing in place', '')}


def _refused(i, noun, reason):
    return PPYoloHipError('%s%s: %s' % (_NOUNS[noun][0], '' if i is None else ' %d' % i, reason))


def check_image(i, t, device, noun='source', grey=False, bound=False, host=False):
    """THE in-place image rule: a uint8 tensor [h,w,3] on `device` with pixel stride 3, channel stride 1 and rows that do not
    overlap, any row pitch (a decoder output, a crop `big[3:3+h, 5:5+w]`).  grey: [h,w] with pixel stride 1 passes too.
    bound: both sides in 1..65535 (otherwise at least 1).  host: a CPU tensor passes once dtype and shape are right, whatever
    its strides: the caller uploads or packs it by value.  i: the item's index, or None.  Returns t.  (Every call of the
    pipeline runs this once per image: the passing path builds no message.)"""
    layouts = '[h, w, 3] or [h, w] (grey)' if grey else '[h, w, 3]'
    if not isinstance(t, torch.Tensor):
        raise _refused(i, noun, 'expected a uint8 tensor %s, got %s' % (layouts, type(t).__name__))
    if t.dtype != torch.uint8:
        raise _refused(i, noun, 'dtype %s, expected uint8' % t.dtype)
    shape = t.shape
    pix = 3 if len(shape) == 3 and shape[2] == 3 else 1 if grey and len(shape) == 2 else 0
    if not pix:
        raise _refused(i, noun, 'shape %s, expected a uint8 image %s' % (tuple(shape), layouts))
    h, w = shape[0], shape[1]
    if h < 1 or w < 1 or (bound and (h > 65535 or w > 65535)):
        raise _refused(i, noun, '%d x %d, width and height must be %s' % (w, h, 'in 1..65535' if bound else 'at least 1'))
    if host and t.device.type == 'cpu':
        return t
    strides = t.stride()
    if strides[1] != pix or (pix == 3 and strides[2] != 1) or (h > 1 and strides[0] < pix * w):
        raise _refused(i, noun, 'strides %s: %s needs pixel stride %d%s and rows that do not overlap (any row pitch)%s'
                       % (tuple(strides), _NOUNS[noun][1], pix, ', channel stride 1' if pix == 3 else '', _NOUNS[noun][2]))
    if not same_device(t.device, device):
        raise _refused(i, noun, 'lives on %s, not on %s where the kernels would touch it: nothing is copied silently, move it '
                       'there (`.to(device)`)' % (t.device, device))
    return t


def check_outputs(out, shapes, device):
    """A decoder's `out=` list: one uint8 device tensor of exactly [h, w, 3] per image, each under the in-place rule."""
    if len(out) != len(shapes):
        raise PPYoloHipError('%d output tensors for %d images' % (len(out), len(shapes)))
    for i, (t, (h, w)) in enumerate(zip(out, shapes)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.uint8 or tuple(t.shape) != (h, w, 3):
            raise PPYoloHipError('output %d must be a uint8 device tensor [%d, %d, 3]' % (i, h, w))
        check_image(i, t, device, 'output')


# ---- staging ----------------------------------------------------------------------------------------------------------------
def _recorded_event():
    ev = torch.cuda.Event()
    ev.record()
    return ev


class Staging(object):
    """One pinned, growing host buffer and the event recorded after the last copy out of it.  initial: its first size in bytes;
    it grows to factor * nbytes and never shrinks.  Pinned only for a cuda device with CUDA available; on the CPU there is no
    event either (event: a callable that returns a recorded event, for tests)."""

    def __init__(self, device, initial, factor=1, event=None):
        self.device = torch.device(device)
        self.initial, self.factor = initial, factor
        self.cuda = self.device.type == 'cuda' and torch.cuda.is_available()
        self._event = event if event is not None else _recorded_event if self.cuda else None
        self.buffer = None
        self.busy = None

    def wait(self):
        """Wait on the host for the last copy out of the buffer (not for the launches behind it)."""
        if self.busy is not None:
            self.busy.synchronize()

    def acquire(self, nbytes):
        self.wait()
        self.busy = None
        if self.buffer is None or self.buffer.numel() < nbytes:
            t = torch.empty(max(self.factor * nbytes, self.initial), dtype=torch.uint8)
            self.buffer = t.pin_memory() if self.cuda else t
        return self.buffer

    def copy(self, nbytes):
        """The first nbytes -> a fresh tensor on the device, non-blocking on the current stream; record() must follow."""
        blob = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        blob.copy_(self.buffer[:nbytes], non_blocking=True)
        return blob

    def record(self):
        self.busy = self._event() if self._event is not None else None

    def upload(self, nbytes):
        blob = self.copy(nbytes)
        self.record()
        return blob


class StagingRing(object):
    """Two Staging slots used in turn, so the host stage of the next batch overlaps the copy and the kernels of this one.  A
    slot is HELD from take() until its batch has been copied to the device (uploading) or release()d; the generation tells a
    batch whose slot has been handed on.  take() and uploading() may run on two threads."""

    def __init__(self, device, initial, stage='host', event=None):
        self.slots = (Staging(device, initial, event=event), Staging(device, initial, event=event))
        self.stage = stage              # what the refusal calls the caller's host half
        self._held = [False, False]     # handed out to a batch that has not been uploaded or released yet
        self._gen = [0, 0]              # how many batches each slot has been handed to
        self._turn = 0
        self._lock = threading.Lock()

    def take(self, nbytes):
        """-> (slot, gen, buffer of at least nbytes), after the last copy out of that buffer."""
        with self._lock:
            s = self._turn if not self._held[self._turn] else self._turn ^ 1
            if self._held[s]:
                raise PPYoloHipError('both staging buffers belong to batches that wait for reconstruct(): the %s stage may '
                                     'run at most two batches ahead; reconstruct() or release() one first' % self.stage)
            self._held[s] = True
            self._gen[s] += 1
            gen = self._gen[s]
            self._turn = s ^ 1
        return s, gen, self.slots[s].acquire(nbytes)

    def release(self, slot, gen):
        """Hand a slot back without an upload; nothing happens if it has moved on to a later batch."""
        with self._lock:
            if self._gen[slot] == gen:
                self._held[slot] = False

    @contextlib.contextmanager
    def uploading(self, slot, gen):
        """Brackets "pack the table, copy(), enqueue what still reads the host buffer": yields the slot's Staging once its last
        copy is done (the same batch again: that copy still reads the table), then records the event and hands the slot back.
        An exception inside leaves the slot held: the batch never reached the device."""
        with self._lock:
            if self._gen[slot] != gen:
                raise PPYoloHipError('stale HostBatch: its staging buffer has been handed to a later batch')
            self._held[slot] = True         # (again, when the same batch is uploaded a second time)
        st = self.slots[slot]
        st.wait()
        try:
            yield st
        finally:
            st.record()                     # (after an exception too: a copy may already be in flight)
        with self._lock:
            self._held[slot] = False


# ---- the decoders' host stage -----------------------------------------------------------------------------------------------
class HostPool(object):
    """The thread pool of a decoder's host stage: min(threads or 16, items of the call) workers, never more than 16, never
    derived from the machine's CPU count; no executor at all while one worker is enough."""

    def __init__(self, threads, prefix):
        if threads is not None and threads < 1:
            raise PPYoloHipError('threads must be >= 1')
        self.threads = None if threads is None else min(int(threads), MAX_THREADS)
        self.prefix = prefix
        self.executor = None

    def map(self, fn, n):
        """[fn(0), ..., fn(n - 1)], in index order; a worker's exception is raised here."""
        if min(self.threads or MAX_THREADS, n) <= 1:
            return [fn(i) for i in range(n)]
        if self.executor is None:
            self.executor = ThreadPoolExecutor(max_workers=self.threads or MAX_THREADS, thread_name_prefix=self.prefix)
        return list(self.executor.map(fn, range(n)))


class ImreadMixin(object):
    """cv2's two single-image calls on top of decode(list)."""

    def imdecode(self, buf):
        return self.decode([buf])[0]

    def imread(self, path):
        return self.decode([path])[0]
