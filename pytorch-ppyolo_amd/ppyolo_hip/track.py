"""Tracking across frames: the rows of forward_padded get an identity that lasts from frame to frame, on the device, with the
tracks' state in a device buffer (csrc/track.hip; include/ppyolo_hip.h has the contract).

    from ppyolo_hip.track import Tracker
    tracker = Tracker(streams=1, device='cuda')
    for frame in frames:
        dets, count, _ = model.forward_padded(pre(frame), im_size)
        rows, n, ids, src, hits = tracker.update(dets, count)          # all on the device, no host synchronisation

ByteTrack-shaped: rows with score >= high_thresh are matched to the tracked and lost tracks, rows between low_thresh and high_thresh
rescue tracked objects, an unmatched row with score >= new_thresh opens a track that is reported from its second frame on (from
the first in the stream's first frame), a track unseen for more than max_lost frames is dropped.  Not built: Hungarian assignment
(greedy matching on a strict order instead), appearance features, camera-motion compensation."""
import torch

from . import _lib, ops
from ._lib import PPYoloHipError, TRACK_MAX_ROWS, TRACK_MAX_TRACKS


def _number(name, v):
    try:
        v = float(v)
    except (TypeError, ValueError):
        raise PPYoloHipError('%s=%r: expected a number' % (name, v))
    if v != v:
        raise PPYoloHipError('%s is NaN' % name)
    return v


class Tracker(object):
    """The tracks of `streams` independent streams of frames.

    max_tracks: slots per stream (1..1024); a row that would open a track while every slot is taken is skipped and counted in the
    state's header.  high_thresh / low_thresh: the two score levels; new_thresh: the score that opens a track (None: high_thresh +
    0.1).  match_thresh: the IoU a pair must EXCEED in stage 1 (high rows x tracked and lost tracks), stage 2 (low rows x tracked
    tracks) and stage 3 (high rows x new tracks).  max_lost: frames a track is kept without a match.  class_agnostic: match
    across class ids."""

    def __init__(self, streams, device, max_tracks=256, high_thresh=0.6, low_thresh=0.1, new_thresh=None, match_thresh=(0.2, 0.5, 0.3),
                 max_lost=30, class_agnostic=False):
        try:
            self.streams, self.max_tracks, max_lost = int(streams), int(max_tracks), int(max_lost)
        except (TypeError, ValueError):
            raise PPYoloHipError('streams=%r, max_tracks=%r, max_lost=%r: expected integers' % (streams, max_tracks, max_lost))
        if not 1 <= self.streams <= 65535:
            raise PPYoloHipError('streams = %d, supported: 1..65535' % self.streams)
        if not 1 <= self.max_tracks <= TRACK_MAX_TRACKS:
            raise PPYoloHipError('max_tracks = %d, supported: 1..%d' % (self.max_tracks, TRACK_MAX_TRACKS))
        if max_lost < 0:
            raise PPYoloHipError('max_lost = %d, must be at least 0' % max_lost)
        high = _number('high_thresh', high_thresh)
        try:
            match = [_number('match_thresh[%d]' % i, v) for i, v in enumerate(match_thresh)]
        except TypeError:
            raise PPYoloHipError('match_thresh=%r: expected the IoU thresholds of stages 1, 2 and 3' % (match_thresh,))
        if len(match) != 3:
            raise PPYoloHipError('match_thresh=%r: expected the IoU thresholds of stages 1, 2 and 3' % (match_thresh,))
        self.params = _lib.TrackParams(high, _number('low_thresh', low_thresh),
                                       high + 0.1 if new_thresh is None else _number('new_thresh', new_thresh),
                                       (_lib.c_float * 3)(*match), max_lost, 1 if class_agnostic else 0)
        self.device = torch.device(device)
        self._state = ops.track_state(self.streams, self.max_tracks, self.device)
        self._stride = self._state.numel() // self.streams

    def update(self, dets, count):
        """dets float32 [streams, K, 6] and count int32 [streams] on the device, as forward_padded returns them (count[i] < 0:
        stream i has no frame in this call and keeps its state).  Returns (rows float32 [streams, max_tracks, 6] = (class, score,
        the track's box) in forward_padded's format, count int32 [streams], ids, src = the row of dets, hits int32 [streams,
        max_tracks], -1 padding): the tracks seen in this frame, by id.  New tensors each call; stream-ordered, no host
        synchronisation."""
        if not (torch.is_tensor(dets) and dets.dim() == 3 and dets.shape[2] == 6 and dets.dtype == torch.float32):
            raise PPYoloHipError('dets: expected a float32 tensor [streams, K, 6], got %s' % (
                '%s %s' % (dets.dtype, tuple(dets.shape)) if torch.is_tensor(dets) else type(dets).__name__))
        n, K = dets.shape[0], dets.shape[1]
        if n != self.streams:
            raise PPYoloHipError('dets has %d streams, the tracker %d' % (n, self.streams))
        if not 1 <= K <= TRACK_MAX_ROWS:
            raise PPYoloHipError('K = %d rows per frame, supported: 1..%d' % (K, TRACK_MAX_ROWS))
        if not (torch.is_tensor(count) and count.dtype == torch.int32 and tuple(count.shape) == (n,)):
            raise PPYoloHipError('count: expected an int32 tensor [%d]' % n)
        T = self.max_tracks
        out = (torch.empty((n, T, 6), dtype=torch.float32, device=self.device), torch.empty((n,), dtype=torch.int32, device=self.device),
               torch.empty((n, T), dtype=torch.int32, device=self.device), torch.empty((n, T), dtype=torch.int32, device=self.device),
               torch.empty((n, T), dtype=torch.int32, device=self.device))
        ops.track_update(dets.contiguous(), count.contiguous(), self.params, self._state, T, *out)
        return out

    def reset(self, streams=None):
        """Forget the tracks of the given streams (None: all): their state is zero-filled on the current stream."""
        if streams is None:
            self._state.zero_()
            return
        for i in streams:
            i = int(i)
            if not 0 <= i < self.streams:
                raise PPYoloHipError('stream %d: the tracker has streams 0..%d' % (i, self.streams - 1))
            self._state[i * self._stride:(i + 1) * self._stride].zero_()

    def state(self):
        """A host copy of the state: int32 numpy [streams, 4 + 28 max_tracks], the layout of include/ppyolo_hip.h (float fields by
        their bits).  Synchronises; for tests."""
        return self._state.cpu().numpy().view('<i4').reshape(self.streams, -1)
