"""Test-time augmentation: the detector runs on the whole image at several network input sides, plain and mirrored, and the rows
of all those views are fused on the device by weighted boxes fusion (csrc/fuse_views.hip).

    from ppyolo_hip.tta import TtaDetector
    tta = TtaDetector(model, cfg, scales=(512, 608, 704), hflip=True)     # fusion at IoU > 0.55, every view weighs 1
    dets, count, src, members = tta([frame])                             # forward_padded's row format, all on the device

The view plan (plan_tta_views) is pure Python and needs no device.  Not built: tiles combined with flips (the table format allows
it), class-agnostic fusion, a confidence rule other than ensemble_boxes' 'avg', vertical flips."""
import numpy as np
import torch

from . import ops
from .hostio import Staging
from ._lib import MERGE_MAX_KEEP, MERGE_MAX_ROWS, PPYoloHipError


def plan_tta_views(sizes, scales, hflip=True, batch=8):
    """[(h, w)] of a batch -> the view table's rows as (image, scale index, flipped, mirror_w), scale after scale; in a scale
    image after image, the plain view before the mirrored one (mirror_w = the image's width), and behind them repeats of the
    scale's first view marked as padding (image = -1) up to a multiple of `batch`: the views of one scale run in chunks of
    exactly `batch`, so one plan of the model per scale serves every call."""
    sizes = [(int(h), int(w)) for h, w in sizes]
    batch = int(batch)
    if not sizes:
        raise PPYoloHipError('empty batch')
    if batch < 1:
        raise PPYoloHipError('batch=%r: must be at least 1' % (batch,))
    rows = []
    for si in range(len(scales)):
        one = [(i, si, f, w if f else 0) for i, (h, w) in enumerate(sizes) for f in ((0, 1) if hflip else (0,))]
        rows += one + [(-1, si, 0, 0)] * (-len(one) % batch)
    return rows


class TtaDetector(object):
    """Detection with flipped and multi-scale views, fused.

    model: a PPYOLO on the device, cfg: its configuration.  scales: the network input sides; every scale is a Preprocessor of its
    own and a plan of its own in the model.  hflip: also run every scale mirrored; the mirrored view is DEFINED as the network
    input mirrored along W after pre-processing (torch.flip of the [n, 3, S, S] tensor), so the pre-process launches are those of
    the plain view.  weights: per scale one weight, or one per (scale, flip) as a nested sequence [len(scales)][1 or 2]; None:
    every view weighs 1.  thresh: a row joins a cluster whose fused box it meets with an IoU strictly above it.  score_thresh: rows
    below it do not enter the fusion (None: the configured NMS's post_threshold or score_threshold); keep_top_k: rows per image of
    the result (None: the configuration's).  batch: views per forward_padded call."""

    def __init__(self, model, cfg, scales=(608,), hflip=True, weights=None, thresh=0.55, score_thresh=None, keep_top_k=None, batch=8):
        from .preprocess import Preprocessor
        self.model = model
        try:
            self.scales = tuple(int(s) for s in scales)
        except TypeError:
            raise PPYoloHipError('scales=%r: expected a sequence of network input sides' % (scales,))
        if not self.scales:
            raise PPYoloHipError('scales=%r: at least one network input side is needed' % (scales,))
        stride = max(getattr(cfg, 'head', {}).get('downsample', [32]))
        for s in self.scales:
            if s < stride or s % stride:
                raise PPYoloHipError('scale %d: the model plans input sides that are positive multiples of %d (its coarsest stride)'
                                     % (s, stride))
        self.hflip = bool(hflip)
        nf = 2 if self.hflip else 1
        if weights is None:
            weights = [[1.0] * nf] * len(self.scales)
        weights = [list(w) if isinstance(w, (list, tuple, np.ndarray)) else [w] * nf for w in weights]
        if len(weights) != len(self.scales) or any(len(w) != nf for w in weights):
            raise PPYoloHipError('weights: expected %d rows (one per scale) of %d values (plain%s)'
                                 % (len(self.scales), nf, ', mirrored' if self.hflip else ''))
        self.weights = np.array(weights, dtype=np.float32).reshape(len(self.scales), nf)
        if not (np.isfinite(self.weights) & (self.weights > 0)).all():
            raise PPYoloHipError('weights=%r: every weight must be finite and positive' % (weights,))
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
        self.batch = int(batch)
        if self.batch < 1:
            raise PPYoloHipError('batch=%r: must be at least 1' % (batch,))
        self.device = next(model.parameters()).device
        self.pre = [Preprocessor(cfg, s, self.device) for s in self.scales]
        self.views = None               # [(image or -1, input side, flipped)] of the last call: the view table's rows
        self._staging = Staging(self.device, 1 << 12, factor=2)
        self._ws = None
        self._keep = None               # what the launches in flight read

    def __call__(self, images):
        """images: uint8 [h, w, 3] device tensors (read in place, hostio.check_image's rule) or numpy arrays (uploaded).  Returns
        (dets float32 [n, keep_top_k, 6] = (class, confidence, fused box), count int32 [n], src int32 [n, keep_top_k, 2] = (view,
        row) of the cluster's first member, members int32 [n, keep_top_k], -1 padding) on the device, stream-ordered, with no host
        synchronisation; view indexes self.views."""
        from .resize import device_source
        from .tiles import preprocess_views
        images = list(images)
        if not images:
            raise PPYoloHipError('empty batch')
        dev = [device_source(i, im, self.device) for i, im in enumerate(images)]
        n = len(dev)
        sizes = [(t.shape[0], t.shape[1]) for t in dev]
        plan = plan_tta_views(sizes, self.scales, self.hflip, self.batch)
        V = len(plan)
        table = ops.fuse_views_table([(i, 0, 0, mw) for i, si, f, mw in plan])
        weight = np.array([self.weights[si, f] for i, si, f, mw in plan], dtype=np.float32)
        im_size = np.array([sizes[max(i, 0)] for i, si, f, mw in plan], dtype=np.float32)      # a padding view repeats image 0
        cur = torch.cuda.current_stream(self.device)
        for t in dev:                   # memory another stream's decoder may own
            t.record_stream(cur)
        # one pinned upload per call: the view table, the weights, then the im_size rows of every chunk
        buf = self._staging.acquire(28 * V)
        buf[:16 * V].view(torch.int32).copy_(torch.from_numpy(table).reshape(-1))
        buf[16 * V:20 * V].view(torch.float32).copy_(torch.from_numpy(weight))
        buf[20 * V:28 * V].view(torch.float32).copy_(torch.from_numpy(im_size).reshape(-1))
        blob = self._staging.upload(28 * V)
        d_table = blob[:16 * V].view(torch.int32).view(V, 4)
        d_weight = blob[16 * V:20 * V].view(torch.float32)
        d_sizes = blob[20 * V:28 * V].view(torch.float32).view(V, 2)
        all_dets, all_count = None, torch.empty((V,), dtype=torch.int32, device=self.device)
        lo = 0
        for si, pre in enumerate(self.pre):
            x, _ = preprocess_views(pre, dev, d_sizes[:n])
            if self.hflip:              # image-major: plain, mirrored
                x = torch.stack([x, torch.flip(x, dims=[3])], dim=1).reshape((2 * n,) + tuple(x.shape[1:]))
            tail = -x.shape[0] % self.batch
            if tail:
                x = torch.cat([x, x[:1].expand((tail,) + tuple(x.shape[1:]))])
            for c in range(0, x.shape[0], self.batch):
                dets, count, _ = self.model.forward_padded(x[c:c + self.batch].contiguous(), d_sizes[lo:lo + self.batch])
                if all_dets is None:
                    all_dets = torch.empty((V,) + tuple(dets.shape[1:]), dtype=torch.float32, device=self.device)
                # forward_padded returns the executor's own buffers: the next chunk overwrites them
                all_dets[lo:lo + self.batch].copy_(dets)
                all_count[lo:lo + self.batch].copy_(count)
                lo += self.batch
        K = all_dets.shape[1]
        out_dets = torch.empty((n, self.keep_top_k, 6), dtype=torch.float32, device=self.device)
        out_count = torch.empty((n,), dtype=torch.int32, device=self.device)
        out_src = torch.empty((n, self.keep_top_k, 2), dtype=torch.int32, device=self.device)
        out_members = torch.empty((n, self.keep_top_k), dtype=torch.int32, device=self.device)
        need = 64 * n * min(V * K, MERGE_MAX_ROWS)      # ppy_fuse_views_workspace_bytes
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(max(need, 1 << 16), dtype=torch.uint8, device=self.device)
        self._ws.record_stream(cur)
        ops.fuse_views(all_dets, all_count, table, d_table, weight, d_weight, n, self.thresh, self.score_thresh, self.keep_top_k,
                       out_dets, out_count, out_src, out_members, ws=self._ws)
        self.views = [(i, self.scales[si], bool(f)) for i, si, f, mw in plan]
        self._keep = (dev, blob, all_dets, all_count, self._ws)
        return out_dets, out_count, out_src, out_members
