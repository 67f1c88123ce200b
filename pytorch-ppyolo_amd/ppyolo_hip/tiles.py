"""Tiled (sliced) inference on large images: the detector runs on overlapping full-size tiles at native resolution plus once on
the whole image, and the rows of all those views are merged on the device (csrc/merge_views.hip).

    from ppyolo_hip.tiles import TiledDetector
    tiled = TiledDetector(model, cfg, target_size=608)                  # tile = 608, overlap 0.2, 'ios' at 0.5
    dets, count, src = tiled([frame_4k])                                # forward_padded's row format, all on the device

The tile plan (tile_origins, plan_views) is pure Python and needs no device."""
import math

import numpy as np
import torch

from . import ops
from .hostio import Staging
from ._lib import MERGE_MAX_KEEP, MERGE_MAX_ROWS, MERGE_METRIC, PPYoloHipError


def tile_origins(L, T, overlap):
    """One axis of length L >= 1 cut into tiles of side T >= 1 with 0 <= overlap < 1 -> (origins, extent).  L <= T: one tile of
    extent L at 0.  Else the stride is max(1, floor(T * (1 - overlap))): origins 0, s, 2s, ... while o + T < L, then a last
    origin L - T.  Every tile is full-size; the last one is shifted back, never cut."""
    L, T = int(L), int(T)
    overlap = float(overlap)
    if L < 1 or T < 1:
        raise PPYoloHipError('tile_origins: length %d and tile %d must be at least 1' % (L, T))
    if not 0.0 <= overlap < 1.0:
        raise PPYoloHipError('tile_origins: overlap=%r must be in [0, 1)' % (overlap,))
    if L <= T:
        return [0], L
    s = max(1, int(math.floor(T * (1.0 - overlap))))
    origins, o = [], 0
    while o + T < L:
        origins.append(o)
        o += s
    origins.append(L - T)
    return origins, T


def plan_views(h, w, tile, overlap, full_view=True):
    """The views of one h x w image as (ox, oy, vw, vh): first the whole image, if full_view is set and the image is larger than
    one tile on some axis, then the tiles in row-major order (y outer, x inner).  An image that is a single tile yields that one
    view only."""
    xs, vw = tile_origins(w, tile, overlap)
    ys, vh = tile_origins(h, tile, overlap)
    views = []
    if full_view and len(xs) * len(ys) > 1:
        views.append((0, 0, int(w), int(h)))
    views += [(ox, oy, vw, vh) for oy in ys for ox in xs]
    return views


def preprocess_views(pre, views, im_size=None, out=None):
    """The views (uint8 [vh, vw, 3] slices of device images, any row pitch) through the configuration's own resize branch and
    the normalisation table of `pre` (a Preprocessor), in one launch and in place: Preprocessor.upload would make every view
    contiguous first.  im_size: the views' own (vh, vw) as a float32 [n, 2] device tensor, where the caller has uploaded it
    already.  Returns (x float32 [n, 3, S, S], im_size)."""
    n, S = len(views), pre.S
    if out is None:
        out = torch.empty((n, 3, S, S), dtype=torch.float32, device=pre.device)
    if pre._pil is not None:          # Pillow's resize: the planner reads pitched sources and keeps them alive
        np_, h_blob, blob, nbytes, ws = pre._pil.plan(views, S, S)
        ops.preprocess_pil_images(np_, h_blob, blob, nbytes, ws, pre.lut, out, swap_rb=pre.to_rgb)
    else:                             # cv2 cubic: the launch takes every image's row pitch
        ops.preprocess_images(views, S, pre.lut, out, swap_rb=pre.to_rgb)
    if im_size is None:
        im_size = torch.tensor([[t.shape[0], t.shape[1]] for t in views], dtype=torch.float32).to(pre.device, non_blocking=True)
    return out, im_size


class TiledDetector(object):
    """Detection on images larger than the network input, by views.

    model: a PPYOLO on the device, cfg: its configuration (the resize branch and the normalisation are the configuration's own),
    target_size: the network input side.  tile: the tile side in image pixels (None: target_size, i.e. native resolution);
    overlap: the fraction of a tile its neighbour repeats; full_view: also run the whole image squashed to the input, which
    sees the objects larger than a tile.  metric / thresh / class_agnostic: the cross-view suppression ('ios' = intersection over
    the smaller box removes the part of an object a tile sees beside the whole object another view sees).  score_thresh: rows
    below it do not enter the merge (None: the configured NMS's post_threshold or score_threshold); keep_top_k: rows per image of
    the result (None: the configuration's).  batch: views per forward_padded call; the last chunk of a call is filled with
    repeats of view 0 marked as padding, so one plan of the model serves every call.

    A tile is an image to the network: the taps of its resize clamp to the tile's own edge, not to the neighbouring pixels."""

    def __init__(self, model, cfg, target_size, tile=None, overlap=0.2, full_view=True, metric='ios', thresh=0.5, score_thresh=None,
                 keep_top_k=None, class_agnostic=False, batch=8):
        from .preprocess import Preprocessor
        self.model = model
        self.target_size = int(target_size)
        self.tile = self.target_size if tile is None else int(tile)
        if self.tile < 1:
            raise PPYoloHipError('tile=%r: must be at least 1' % (tile,))
        self.overlap = float(overlap)
        if not 0.0 <= self.overlap < 1.0:
            raise PPYoloHipError('overlap=%r must be in [0, 1)' % (overlap,))
        self.full_view = bool(full_view)
        if metric not in MERGE_METRIC:
            raise PPYoloHipError("unknown metric %r, known: 'iou', 'ios'" % (metric,))
        self.metric = metric
        self.thresh = float(thresh)
        if self.thresh != self.thresh:
            raise PPYoloHipError('thresh is NaN')
        nms = cfg.nms_cfg
        if score_thresh is None:
            score_thresh = nms['post_threshold'] if nms.get('nms_type', 'matrix_nms') == 'matrix_nms' else nms['score_threshold']
        self.score_thresh = float(score_thresh)
        if self.score_thresh != self.score_thresh:
            raise PPYoloHipError('score_thresh is NaN')
        self.keep_top_k = int(nms['keep_top_k'] if keep_top_k is None else keep_top_k)
        if not 1 <= self.keep_top_k <= MERGE_MAX_KEEP:
            raise PPYoloHipError('keep_top_k = %d, supported: 1..%d' % (self.keep_top_k, MERGE_MAX_KEEP))
        self.class_agnostic = bool(class_agnostic)
        self.batch = int(batch)
        if self.batch < 1:
            raise PPYoloHipError('batch=%r: must be at least 1' % (batch,))
        self.device = next(model.parameters()).device
        self.pre = Preprocessor(cfg, self.target_size, self.device)
        self.views = None               # [(image, ox, oy, vw, vh)] of the last call, padding views excluded
        self._staging = Staging(self.device, 1 << 12, factor=2)
        self._ws = None
        self._keep = None               # what the launches in flight read

    def plan(self, sizes):
        """[(h, w)] -> [(image, ox, oy, vw, vh)] for a batch, image-major."""
        return [(i, ox, oy, vw, vh) for i, (h, w) in enumerate(sizes)
                for ox, oy, vw, vh in plan_views(h, w, self.tile, self.overlap, self.full_view)]

    def chunks(self, views):
        """The plan in chunks of exactly `batch` views: [(view, is_padding)] each; the last one is filled with view 0."""
        padded = [(v, False) for v in views] + [(views[0], True)] * (-len(views) % self.batch)
        return [padded[i:i + self.batch] for i in range(0, len(padded), self.batch)]

    def view_tensors(self, dev, chunk):
        """The chunk's views as slices of the device images (no copy)."""
        return [dev[i][oy:oy + vh, ox:ox + vw] for (i, ox, oy, vw, vh), _ in chunk]

    def __call__(self, images):
        """images: uint8 [h, w, 3] device tensors (read in place, hostio.check_image's rule) or numpy arrays (uploaded).  Returns
        (dets float32 [n, keep_top_k, 6], count int32 [n], src int32 [n, keep_top_k, 2] = (view, row), -1 padding) on the
        device, stream-ordered, with no host synchronisation; view indexes self.views."""
        from .resize import device_source
        images = list(images)
        if not images:
            raise PPYoloHipError('empty batch')
        dev = [device_source(i, im, self.device) for i, im in enumerate(images)]
        n = len(dev)
        views = self.plan([(t.shape[0], t.shape[1]) for t in dev])
        chunks = self.chunks(views)
        V = len(chunks) * self.batch
        table = ops.merge_views_table([(-1 if pad else v[0], v[1], v[2]) for ch in chunks for v, pad in ch])
        sizes = np.array([[v[4], v[3]] for ch in chunks for v, _ in ch], dtype=np.float32)      # every view's own (vh, vw)
        cur = torch.cuda.current_stream(self.device)
        for t in dev:                   # memory another stream's decoder may own
            t.record_stream(cur)
        # one pinned upload per call: the view table, then the im_size rows of every chunk
        buf = self._staging.acquire(20 * V)
        buf[:12 * V].view(torch.int32).copy_(torch.from_numpy(table).reshape(-1))
        buf[12 * V:20 * V].view(torch.float32).copy_(torch.from_numpy(sizes).reshape(-1))
        blob = self._staging.upload(20 * V)
        d_table = blob[:12 * V].view(torch.int32).view(V, 3)
        d_sizes = blob[12 * V:20 * V].view(torch.float32).view(V, 2)
        all_dets, all_count = None, torch.empty((V,), dtype=torch.int32, device=self.device)
        for c, ch in enumerate(chunks):
            lo, hi = c * self.batch, (c + 1) * self.batch
            x, im_size = preprocess_views(self.pre, self.view_tensors(dev, ch), d_sizes[lo:hi])
            dets, count, _ = self.model.forward_padded(x, im_size)
            if all_dets is None:
                all_dets = torch.empty((V,) + tuple(dets.shape[1:]), dtype=torch.float32, device=self.device)
            # forward_padded returns the executor's own buffers: the next chunk overwrites them
            all_dets[lo:hi].copy_(dets)
            all_count[lo:hi].copy_(count)
        K = all_dets.shape[1]
        out_dets = torch.empty((n, self.keep_top_k, 6), dtype=torch.float32, device=self.device)
        out_count = torch.empty((n,), dtype=torch.int32, device=self.device)
        out_src = torch.empty((n, self.keep_top_k, 2), dtype=torch.int32, device=self.device)
        need = 32 * n * min(V * K, MERGE_MAX_ROWS)      # ppy_merge_views_workspace_bytes
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(max(need, 1 << 16), dtype=torch.uint8, device=self.device)
        self._ws.record_stream(cur)
        ops.merge_views(all_dets, all_count, table, d_table, n, self.metric, self.thresh, self.score_thresh, self.class_agnostic,
                        self.keep_top_k, out_dets, out_count, out_src, ws=self._ws)
        self.views = views
        self._keep = (dev, blob, all_dets, all_count, self._ws)
        return out_dets, out_count, out_src
